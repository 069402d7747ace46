"""CPU: batchnorm.freeze_batch_norm / unfreeze_batch_norm and the route decision of archs.BasicBlock.  No kernel runs."""
import itertools

import pytest
import torch
import torch.nn as nn


def _model(pkg):
    blk = pkg.archs.BasicBlock(8, 8)
    return nn.Sequential(blk, nn.Sequential(nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4))), blk


def _bns(m):
    return [x for x in m.modules() if isinstance(x, nn.modules.batchnorm._BatchNorm)]


def test_freeze_counts_layers_and_survives_train(pkg):
    m, blk = _model(pkg)
    assert pkg.batchnorm.freeze_batch_norm(m) == 3
    assert all(not b.training for b in _bns(m))
    assert m.train() is m
    assert all(not b.training for b in _bns(m)) and m.training and blk.training and m[1][0].training
    m.eval(); m.train(True)
    assert all(not b.training for b in _bns(m))
    assert all(p.requires_grad for b in _bns(m) for p in (b.weight, b.bias))          # the affine stays trainable by default
    assert pkg.batchnorm.freeze_batch_norm(m) == 3                                       # idempotent
    assert blk.bn1.train() is blk.bn1 and not blk.bn1.training


def test_unfreeze_restores_modes_and_requires_grad(pkg):
    m, blk = _model(pkg)
    blk.bn2.weight.requires_grad_(False)                                                 # was already off before the freeze
    m.train()
    assert pkg.batchnorm.freeze_batch_norm(m, freeze_affine=True) == 3
    assert not any(p.requires_grad for b in _bns(m) for p in (b.weight, b.bias))
    assert pkg.batchnorm.unfreeze_batch_norm(m) == 3
    assert all(b.training for b in _bns(m))                                              # each takes its parent's mode
    assert blk.bn1.weight.requires_grad and blk.bn1.bias.requires_grad and blk.bn2.bias.requires_grad and not blk.bn2.weight.requires_grad
    m.eval()
    assert not any(b.training for b in _bns(m))
    m.train()
    assert all(b.training for b in _bns(m))
    assert pkg.batchnorm.unfreeze_batch_norm(m) == 0
    bn = nn.BatchNorm2d(4)
    assert pkg.batchnorm.freeze_batch_norm(bn) == 1 and not bn.train().training
    assert pkg.batchnorm.unfreeze_batch_norm(bn) == 1 and bn.train().training


def test_frozen_layers_keep_their_state_dict_and_deepcopy(pkg):
    import copy
    import pickle
    m, _ = _model(pkg)
    keys = list(m.state_dict())
    pkg.batchnorm.freeze_batch_norm(m)
    assert list(m.state_dict()) == keys
    c = copy.deepcopy(m)
    c.train()
    assert all(not b.training for b in _bns(c))
    q = pickle.loads(pickle.dumps(m))                                                    # torch.save(model), spawn
    q.train()
    assert all(not b.training for b in _bns(q)) and all(b.train.args[0] is b for b in _bns(q))
    assert pkg.batchnorm.unfreeze_batch_norm(q) == 3 and all(b.training for b in _bns(q.train()))


WANT = {   # (block.training, batch norms in train mode, grad enabled) -> route
    (True, True, True): 'train', (True, True, False): 'train',
    (True, False, True): 'frozen', (True, False, False): 'frozen',
    (False, True, True): 'mixed', (False, True, False): 'cached_eval',
    (False, False, True): 'frozen', (False, False, False): 'cached_eval',
}


@pytest.mark.parametrize('block_train,bn_train,grad', list(itertools.product((True, False), repeat=3)))
def test_basic_block_route(pkg, block_train, bn_train, grad):
    blk = pkg.archs.BasicBlock(8, 8)
    blk.train(block_train)
    blk.bn1.train(bn_train); blk.bn2.train(bn_train)
    with torch.set_grad_enabled(grad):
        assert blk._route() == WANT[(block_train, bn_train, grad)]


def test_basic_block_route_mixed_states(pkg):
    blk = pkg.archs.BasicBlock(8, 8)
    blk.train(); blk.bn2.eval()
    assert blk._route() == 'mixed'                                                       # one batch norm frozen
    blk.bn1.eval()
    assert blk._route() == 'frozen'
    blk.bn1 = nn.BatchNorm2d(8, affine=False).eval()
    assert blk._route() == 'mixed'                                                       # a non-affine batch norm cannot be folded with gradients
    odd = pkg.archs.BasicBlock(6, 6).train()
    odd.bn1.eval(); odd.bn2.eval()
    assert odd._route() == 'mixed'                                                       # the frozen node runs whole channel quads
    blk.bn1 = nn.BatchNorm2d(8, track_running_stats=False).eval()
    blk.bn2.train()
    assert blk._route() == 'train'                                                       # no running statistics: batch statistics in any mode

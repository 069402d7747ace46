"""Throughput of the rows beside the headline path (per-op A11/A12), one JSON
object per line.  Not the graded metric (that is bench.py); these are the measurements DESIGN.md quotes for them.
Usage (GPU box): python tools/bench_extra.py            (every row)
                 python tools/bench_extra.py sw         (only the sliding-window pipeline rows)"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S  # noqa: E402

dev = torch.device('cuda')


def timed(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def event_ms(fn, warm, n):
    """HIP-event time of one fn() in ms (fn only enqueues)."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def sliding_window_rows(G):
    """C5 end to end from the in-memory uint8 image: one 2048^2 image, patch 1024, overlap 0.5, inference at 512^2."""
    A, ops, L = S.aerial_image_segmentation_api, S.ops, S._lib
    cfg = dict(patch_size=1024, input_w=512, input_h=512, patch_overlap=0.5, num_classes=3)
    img = np.random.default_rng(5).integers(0, 256, (2048, 2048, 3), dtype=np.uint8)

    def host_path():
        full, patches, masks = A.get_patched_input('image', cfg, False, imread=lambda p: img)
        return A.segmentation_inference_full(G, full, patches, masks, cfg, False, batch_size=12)[0]
    t_host = timed(host_path, 1, 2)
    t_dev = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=False), 1, 3)
    t_dedupe = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=True), 1, 3)
    # the opt-in bf16x1 precision (ops.infer_precision: an approximation), same image and geometry, alternated with the fp32 rows
    t_dev_x1 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=False, precision='bf16x1'), 1, 3)
    t_dedupe_x1 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=True, precision='bf16x1'), 1, 3)
    t_dev2 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=False), 1, 3)
    t_dedupe2 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=True), 1, 3)
    m32 = A.segment_image(G, img, cfg, batch_size=12, dedupe=True)
    mx1 = A.segment_image(G, img, cfg, batch_size=12, dedupe=True, precision='bf16x1')
    differ = float(np.mean([np.mean(a != b) for a, b in zip(m32, mx1)]))
    out = [{'what': 'C5 one 2048^2 uint8 image -> 3 class masks, patch 1024 / overlap 0.5 / inference 512^2, batch 12, from the in-memory array',
            's_per_image_host_gather_and_merge': round(t_host, 3), 's_per_image_segment_image': round(t_dev, 4),
            's_per_image_segment_image_dedupe': round(t_dedupe, 4)},
           {'what': "C5 the same image with precision='bf16x1' (bf16 operand rounding in the BasicBlock 3x3 stride-1 convs; seeded, untrained model), "
                    'fp32 rows repeated after it in the same process',
            's_per_image_segment_image_bf16x1': round(t_dev_x1, 4), 's_per_image_segment_image_dedupe_bf16x1': round(t_dedupe_x1, 4),
            's_per_image_segment_image_fp32_again': round(t_dev2, 4), 's_per_image_segment_image_dedupe_fp32_again': round(t_dedupe2, 4),
            'fraction_of_mask_bytes_that_differ_from_fp32': round(differ, 6)}]
    # the two kernels alone (HIP events), for all 36 patches and for the 9 distinct ones, against the forwards they surround
    dimg = torch.from_numpy(img).to(dev)
    org36 = A.patch_origins(2048, 2048, 1024, 0.5)
    org9, w9 = A.unique_origins(org36)
    consts = ops._sw_norm_consts()
    row = {'what': 'C5 sliding-window kernels alone (HIP events) and the batch-12 forwards between them, input resident'}
    for name, org, wts in (('36', org36, [1] * 36), ('9', org9, w9)):
        host, devo = ops._sw_origins(org, dev)
        n = len(org)
        x = ops.new_nhwc(n, 3, 512, 512, dev)
        probs = ops.new_nhwc(n, 3, 512, 512, dev)
        probs.copy_(torch.rand(n, 3, 512, 512, generator=torch.Generator().manual_seed(9)))
        wdev = torch.tensor(wts, dtype=torch.int32).to(dev)
        masks = torch.empty((3, 2048, 2048), dtype=torch.uint8, device=dev)
        ms_g = event_ms(lambda: L.call('ssg_sw_gather_patches_u8_f32', L.ptr(dimg), 2048, 2048, L.ptr(devo), L.ptr(host), n, 1024, 512,
                                       *(consts + [L.ptr(x), L.stream_ptr()])), 10, 1000)
        ms_m = event_ms(lambda: L.call('ssg_sw_merge_masks_f32_u8', L.ptr(probs), 4, n, 3, 512, L.ptr(devo), L.ptr(host), L.ptr(wdev),
                                       1024, 2048, 2048, L.ptr(masks), L.stream_ptr()), 10, 1000)
        row['ms_gather_%s_patches' % name] = round(ms_g, 4)
        row['ms_merge_%s_patches' % name] = round(ms_m, 4)
        row['gather_%s_write_gb_per_s' % name] = round(n * 512 * 512 * 16 / ms_g / 1e6, 1)
        row['merge_%s_read_gb_per_s' % name] = round(n * 512 * 512 * 16 / ms_m / 1e6, 1)
        if n == 36:
            G.eval()
            with torch.no_grad():
                dt = timed(lambda: [ops.sigmoid(G(x[i:i + 12])) for i in range(0, 36, 12)], 1, 3)
            row['ms_36_forwards_batch_12'] = round(dt * 1e3, 2)
            with torch.no_grad(), ops.infer_precision('bf16x1'):
                dt = timed(lambda: [ops.sigmoid(G(x[i:i + 12])) for i in range(0, 36, 12)], 1, 3)
            row['ms_36_forwards_batch_12_bf16x1'] = round(dt * 1e3, 2)
            # where an eval forward's time goes under each precision: HIP-event time of the conv launches by kernel label
            for prec in ('fp32', 'bf16x1'):
                ops.PROFILE = []
                try:
                    with torch.no_grad(), ops.infer_precision(prec):
                        ops.sigmoid(G(x[:12]))
                    torch.cuda.synchronize()
                    by = {}
                    for rec in ops.PROFILE:
                        by[rec[0]] = by.get(rec[0], 0.0) + rec[2].elapsed_time(rec[3])
                finally:
                    ops.PROFILE = None
                row['ms_conv_launches_one_batch_12_forward_%s' % prec] = {k: round(v, 3) for k, v in sorted(by.items(), key=lambda kv: -kv[1])[:8]}
        del x, probs
    out.append(row)
    return out


def main():
    g = torch.Generator().manual_seed(7)
    out = []
    # C5: eval-mode generator over the 36 patches of a 2048^2 image (patches resized to 512^2), batched
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)
    if sys.argv[1:] == ['sw']:
        for o in sliding_window_rows(G):
            print(json.dumps(o), flush=True)
        return
    patches = torch.randn(36, 3, 512, 512, generator=g)
    for bs in (1, 12):
        dt = timed(lambda: S.aerial_image_segmentation_api.infer_patches(G, patches, batch_size=bs), 1, 3)
        out.append({'what': 'C5 sliding-window inference, 36 x 3x512x512 patches, eval-mode G (BN folded), batch %d, incl. H2D/D2H' % bs,
                    'patches_per_s': round(36 / dt, 2), 's_per_image': round(dt, 3)})
    out += sliding_window_rows(G)
    # batch 1 on resident inputs: kernel-by-kernel launches vs hipGraph replay (what the launch path costs at batch 1)
    xb = patches[:1].to(dev)
    G.eval()
    with torch.no_grad():
        dt_eager = timed(lambda: S.ops.sigmoid(G(xb)), 3, 20)
        gr, sin, sout = S.aerial_image_segmentation_api._graph_for(G, xb.shape, dev)
        sin.copy_(xb)
        dt_graph = timed(lambda: gr.replay(), 3, 20)
    out.append({'what': 'C5 one 3x512x512 patch, eval-mode G, input resident: eager launches vs hipGraph replay',
                'ms_eager': round(dt_eager * 1e3, 3), 'ms_graph': round(dt_graph * 1e3, 3)})
    # N1: stage-1 trainer step (G only, BCEDice, weight clamp, Adam with weight decay)
    cfg = {'clip': 0.7, 'num_classes': 3, 'deep_supervision': False}
    model = S.archs.UNet_R_SS_v2(3, 3, False).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
    crit = S.losses.BCEDiceLoss()
    x = torch.randn(16, 3, 512, 512, generator=g); t = (torch.rand(16, 3, 512, 512, generator=g) > 0.5).float()
    loader = [(None, x, t, None, None)]
    import contextlib, io
    def stage1():
        with contextlib.redirect_stdout(io.StringIO()):
            S.train.train(2, cfg, loader, model, crit, opt, None)
    dt = timed(stage1, 2, 4)
    out.append({'what': 'N1 stage-1 trainer step (train.py:68-137), 16 x 3x512x512, fp32, incl. H2D of the batch',
                'images_per_s': round(16 / dt, 2), 'ms_per_step': round(dt * 1e3, 1)})
    del model, opt, G
    torch.cuda.empty_cache()
    # C4: EfficientNet-B4 encoder extract_features fwd+bwd, N=4 @ 1024^2 (fp32 here; the reference defines no B4 U-Net)
    for name, n, hw in (('efficientnet-b0', 16, 512), ('efficientnet-b4', 4, 1024)):
        enc = S.efficientnet_pytorch.EfficientNet.from_name(name).to(dev).train()
        xin = torch.randn(n, 3, hw, hw, generator=g).to(dev)
        def step():
            enc.zero_grad(set_to_none=True)
            f = enc.extract_features(xin)
            f.sum().backward()
        dt = timed(step, 2, 5)
        out.append({'what': 'C4/A10 %s extract_features fwd+bwd, %d x 3x%dx%d, fp32, train mode' % (name, n, hw, hw),
                    'images_per_s': round(n / dt, 2), 'ms_per_step': round(dt * 1e3, 1)})
        del enc
        torch.cuda.empty_cache()
    # A11: xResidualBlock fwd+bwd
    blk = S.xresidualblock.xResidualBlock(64, 64).to(dev).train()
    xin = torch.randn(16, 64, 256, 256, generator=g).to(dev).requires_grad_(True)
    def xres():
        blk.zero_grad(set_to_none=True)
        blk(xin).sum().backward()
    dt = timed(xres, 2, 5)
    out.append({'what': 'A11 xResidualBlock(64,64) fwd+bwd, 16 x 64x256x256', 'ms_per_step': round(dt * 1e3, 2),
                'gb_per_s_of_input_tensor': round(16 * 64 * 256 * 256 * 4 / dt / 1e9, 1)})
    # A12: spectral norm on the discriminator's 8 conv weights (one power iteration each, as a training forward does)
    D = S.models_seg_gan.Discriminator(3, 3, 64, 8, 1024).to(dev).train()
    convs = [m for m in D.modules() if isinstance(m, nn.Conv2d)]
    for m in convs:
        S.spectral_norm.spectral_norm(m)
    hooks = [(next(h for h in m._forward_pre_hooks.values() if isinstance(h, S.spectral_norm.SpectralNorm)), m) for m in convs]

    def sn():
        with torch.no_grad():
            for h, m in hooks:
                h(m, None)
    dt = timed(sn, 2, 10)
    wbytes = sum(m.weight_orig.numel() * 4 for m in convs)
    out.append({'what': 'A12 spectral_norm power iteration + W/sigma on the 8 discriminator conv weights (%.1f MB)' % (wbytes / 1e6),
                'us_total': round(dt * 1e6, 1)})
    for o in out:
        print(json.dumps(o), flush=True)


if __name__ == '__main__':
    main()

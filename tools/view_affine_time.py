"""What the affine view (rotation by any angle, zoom, shear in the view pass) costs: its kernel beside the fixed-size view
on as many outputs, the whole call beside the chain it replaces (full-tile tensor -> affine_grid -> grid_sample), and the label planes
beside grid_sample(mode="nearest") on a float copy.
    python tools/view_affine_time.py [--out profiles/view_affine_time.txt] [--tiles 512] [--size 1024] [--crop 896] [--collections 5]
Device-resident synthetic tiles, 512 tiles of 1024^2 -> 896^2, float16 NCHW.  Timed by HIP events after a 0.25 s spin-up of the same
call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections (their min and max
beside it).  Every yardstick is existing code, timed in the same process as what it is compared with:
  (a) the kernel: sl_normalize_view_affine (the jitter route) at 0 degrees, 45 degrees and the row-sum limit (45 degrees at 1 / z =
      sqrt 2) beside sl_normalize_view on as many outputs.  At 45 degrees the source block of a patch is the bounding box of a rotated
      square: about twice the source pixels per output are read and computed.  The ratio is printed whichever way it falls.
  (b) end to end, fits included, TileAffine(crop, zoom=(0.8, 1.2), shear=(-10, 10), translate=0.05): augment_batch(view=, tensor_format=)
      against augment_batch(tensor_format=) on the full tile followed by affine_grid + grid_sample(bilinear, align_corners=False)
  (c) int64 labels through TileAffine.apply against grid_sample(mode="nearest") on a float32 copy and the cast back
(The chains of (b) and (c) are ANOTHER definition: grid_sample blends float16 values with float weights and pads with zeros, the fused pass
blends bytes with 8-bit weights and pads with the fill byte; nearest rounds a float coordinate.  They are not compared bit for bit; the
largest difference over the pixels whose taps all lie inside the tile is printed.)
One process; it runs under the caller's time limit, and an error ends it before anything further is started on the device."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/view_affine_time.txt")
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--crop", type=int, default=896)
    ap.add_argument("--collections", type=int, default=5)
    args = ap.parse_args()

    sys.path.insert(0, ".")
    import numpy as np
    import torch
    import stainlib_amd
    from stainlib_amd import engine
    from stainlib_amd.tile_view import AFFINE_Q as Q, affine_row_sums
    from tools.synth import synth_tiles

    def collection(fn, reps=20):
        """median ms of `reps` calls timed one by one, after a spin-up"""
        t_spin = time.perf_counter()
        while time.perf_counter() - t_spin < 0.25:
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)

    def timed(fn):
        ms = [collection(fn) for _ in range(args.collections)]
        return statistics.median(ms), min(ms), max(ms)

    def row(label, t):
        return "  %-104s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])

    n, size, crop = args.tiles, args.size, args.crop
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    target = synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy()
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(target)
    rgb = synth_tiles(n, size, size, seed=9)
    M, maxC, status = engine.macenko_fit(rgb)
    assert int((status != 0).sum()) == 0
    Mt, ct = nz._target_on(rgb.device)
    np.random.seed(3)
    ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=rgb.device)
    route = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct, alpha_beta=ab)
    out = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=rgb.device)
    lines = ["device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up; "
             "one process" % (torch.cuda.get_device_name(0), args.collections), ""]

    # ---- (a) the kernel beside the fixed-size view
    lines.append("(a) %d tiles of %d^2 -> %d^2, jitter route -> float16 NCHW" % (n, size, crop))
    np.random.seed(4)
    d3 = torch.from_numpy(stainlib_amd.TileView(crop).draw(n, size, size)).cuda()
    t0 = timed(lambda: engine.normalize_view(rgb, d3, crop, 7, fmt=f16, out=out, **route))
    lines.append(row("sl_normalize_view (crop / flip / rot90, all eight codes)", t0))
    c45 = np.cos(np.pi / 4)
    for label, mat in (("0 degrees (the identity matrix; patches of 63)", (1, 0, 0, 1)),
                       ("45 degrees (patches of 44, about 2 source pixels computed per output)", (c45, -c45, c45, c45)),
                       ("45 degrees at 1 / z = sqrt 2, the row-sum limit (patches of 32, about 4 per output)", (1, -1, 1, 1))):
        win = np.tile([int(np.rint(Q * v)) for v in (size / 2, size / 2) + tuple(mat)], (n, 1)).astype(np.int32)
        dwin, r = torch.from_numpy(win).cuda(), int(affine_row_sums(win).max())
        t1 = timed(lambda: engine.normalize_view_affine(rgb, dwin, crop, r, 255, fmt=f16, out=out, **route))
        lines.append(row("sl_normalize_view_affine at " + label, t1))
        lines.append("    the affine view takes %.2f of the fixed-size view's time" % (t1[0] / t0[0]))

    # ---- (b) end to end against affine_grid + grid_sample
    view = stainlib_amd.TileAffine(crop, zoom=(0.8, 1.2), shear=(-10, 10), translate=0.05)
    np.random.seed(5)
    win = view.draw(n, size, size)
    dwin = torch.from_numpy(win).cuda()
    ws = engine.Workspace()
    full = torch.empty((n, 3, size, size), dtype=torch.float16, device=rgb.device)
    w64 = torch.from_numpy(win.astype(np.float64) / Q).cuda()
    cy, cx, a00, a01, a10, a11 = (w64[:, k] for k in range(6))
    theta = torch.stack([torch.stack([a11 * crop / size, a10 * crop / size, 2 * cx / size - 1], dim=1),
                         torch.stack([a01 * crop / size, a00 * crop / size, 2 * cy / size - 1], dim=1)], dim=1)

    def fused_host():
        return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=win)[0]

    def fused_dev():
        return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]

    def chain():
        x = nz.augment_batch(rgb, ab, out=full, ws=ws, tensor_format=f16)[0]
        grid = torch.nn.functional.affine_grid(theta.to(torch.float16), (n, 3, crop, crop), align_corners=False)
        return torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)

    def inside(k, margin):
        """(k, crop, crop) bool: the pixels of the first k tiles whose position lies `margin` pixels inside the tile"""
        i = torch.arange(crop, device=rgb.device, dtype=torch.float64)
        u, v = (2 * i + 1 - crop)[None, :, None], (2 * i + 1 - crop)[None, None, :]
        Y = cy[:k, None, None] + (a00[:k, None, None] * u + a01[:k, None, None] * v) / 2
        X = cx[:k, None, None] + (a10[:k, None, None] * u + a11[:k, None, None] * v) / 2
        return (Y > margin) & (Y < size - margin) & (X > margin) & (X < size - margin)

    k = min(n, 8)
    m = inside(k, 2.0)[:, None].expand(k, 3, crop, crop)
    diff = float((chain()[:k].float() - fused_host()[:k].float()).abs()[m].max())
    assert torch.equal(fused_host().view(torch.int16).clone(), fused_dev().view(torch.int16))
    tc, th, td = timed(chain), timed(fused_host), timed(fused_dev)
    lines += ["", "(b) augment_batch, fits included; %d tiles of %d^2, %r -> float16 NCHW" % (n, size, view),
              row("chain: augment_batch(tensor_format=) -> affine_grid -> grid_sample(bilinear, zeros)", tc),
              row("fused: augment_batch(view=, tensor_format=), windows on the host (launch sized by their largest row sum)", th),
              row("fused: the same, windows on the device (launch sized by the view's bound)", td),
              "    the fused call takes %.2f (host windows) and %.2f (device windows) of the chain's time; largest |chain - fused| on pixels "
              "2 px inside the tile (first %d tiles) = %.4f (another definition: see the tool's docstring)" % (th[0] / tc[0], td[0] / tc[0], k, diff)]
    del full
    torch.cuda.empty_cache()

    # ---- (c) int64 labels
    labels = torch.randint(0, 6, (n, size // 8, size // 8), device=rgb.device, dtype=torch.int64)
    labels = labels.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).contiguous()        # blobs of 8 x 8
    lout = torch.empty((n, crop, crop), dtype=torch.int64, device=rgb.device)

    def planes_fused():
        return view.apply(labels, dwin, fill=255, out=lout)

    def planes_chain():
        grid = torch.nn.functional.affine_grid(theta.to(torch.float32), (n, 1, crop, crop), align_corners=False)
        return torch.nn.functional.grid_sample(labels[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].long()

    mism = float((planes_chain()[:k] != planes_fused()[:k])[inside(k, 1.0)].float().mean())
    tpc, tpf = timed(planes_chain), timed(planes_fused)
    lines += ["", "(c) int64 labels, %d planes of %d^2 -> %d^2, the windows of (b) on the device" % (n, size, crop),
              row("chain: float32 copy -> affine_grid -> grid_sample(mode='nearest') -> int64", tpc),
              row("fused: TileAffine.apply (sl_view_planes_affine, 8-byte elements)", tpf),
              "    the fused call takes %.2f of the chain's time; share of inside elements that differ (first %d tiles) = %.6f (float "
              "coordinates round differently at element edges)" % (tpf[0] / tpc[0], k, mism)]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

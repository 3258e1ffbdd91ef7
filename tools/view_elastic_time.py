"""What the elastic view (the affine view plus a smooth displacement field in the view pass) costs: its kernel beside the
affine view's on the same rows, the whole call beside the chain it replaces (full-tile tensor -> a per-pixel displacement field ->
grid_sample), and the label planes beside grid_sample(mode="nearest") on a float copy.
    python tools/view_elastic_time.py [--out profiles/view_elastic_time.txt] [--tiles 512] [--size 1024] [--crop 896] [--collections 5]
Device-resident synthetic tiles, 512 tiles of 1024^2 -> 896^2, float16 NCHW.  Timed by HIP events after a 0.25 s spin-up of the same
call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections (their min and max
beside it).  Every yardstick is timed in the same process as what it is compared with:
  (a) the kernel: sl_normalize_view_elastic (the jitter route, cells of 32) at max_d = 0 (a zero field), 2, 4 and 8 -- random fields at
      the bound -- at 0 and 45 degrees, beside sl_normalize_view_affine on the same rows.  At the zero field the two are compared bit for
      bit.  The elastic view loses by its smaller patches -- (63 / 47)^2 more workgroups at the identity with max_d = 8, each staging a
      64 x 64 block all the same -- and by the evaluation of the field per output pixel.  The ratio is printed whichever way it falls.
  (b) end to end, fits included, TileElastic(crop, magnitude=(0, 4), cell=32, zoom=(0.8, 1.2)): augment_batch(view=, tensor_format=)
      against augment_batch(tensor_format=) on the full tile followed by a dense displacement field (affine_grid plus the bilinearly
      upsampled control lattice) and grid_sample(bilinear, align_corners=False)
  (c) int64 labels through TileElastic.apply against grid_sample(mode="nearest") with the grid of (b) on a float32 copy and the cast back
(The chains of (b) and (c) are the work replaced, ANOTHER definition -- a bilinear, not a B-spline, interpolation of the lattice, float
weights, zero padding -- and no reference for bits; nothing of them is compared.)
One process; it runs under the caller's time limit, and an error ends it before anything further is started on the device."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/view_elastic_time.txt")
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
    from stainlib_amd.tile_view import AFFINE_Q as Q, ElasticWindows, affine_row_sums, elastic_grid_shape
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

    n, size, crop, cell = args.tiles, args.size, args.crop, 32
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
    gh, gw = elastic_grid_shape(crop, cell)
    lines = ["device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up; "
             "one process" % (torch.cuda.get_device_name(0), args.collections), ""]

    # ---- (a) the kernel beside the affine view's on the same rows
    lines.append("(a) %d tiles of %d^2 -> %d^2, jitter route -> float16 NCHW, cells of %d" % (n, size, crop, cell))
    c45 = np.cos(np.pi / 4)
    rng = np.random.RandomState(6)
    for label, mat in (("0 degrees", (1, 0, 0, 1)), ("45 degrees", (c45, -c45, c45, c45))):
        win = np.tile([int(np.rint(Q * v)) for v in (size / 2, size / 2) + tuple(mat)], (n, 1)).astype(np.int32)
        dwin, r = torch.from_numpy(win).cuda(), int(affine_row_sums(win).max())
        t0 = timed(lambda: engine.normalize_view_affine(rgb, dwin, crop, r, 255, fmt=f16, out=out, **route))
        lines.append(row("sl_normalize_view_affine at %s" % label, t0))
        ref = out.view(torch.int16).clone()
        for md in (0, 2, 4, 8):
            field = torch.from_numpy(rng.randint(-256 * md, 256 * md + 1, (n, gh, gw, 2)).astype(np.int32)).cuda()
            t1 = timed(lambda: engine.normalize_view_elastic(rgb, dwin, field, crop, cell, r, md, 255, fmt=f16, out=out, **route))
            if md == 0:
                assert torch.equal(out.view(torch.int16), ref), "the zero field is not the affine view"
            lines.append(row("sl_normalize_view_elastic at %s, max_d = %d%s" % (label, md, " (a zero field: the affine view's bits)" if md == 0 else ""), t1))
            lines.append("    the elastic view takes %.2f of the affine view's time" % (t1[0] / t0[0]))
        del ref

    # ---- (b) end to end against a dense displacement field + grid_sample
    view = stainlib_amd.TileElastic(crop, magnitude=(0, 4), cell=cell, zoom=(0.8, 1.2))
    np.random.seed(5)
    win = view.draw(n, size, size)
    dwin = ElasticWindows(torch.from_numpy(win.affine).cuda(), torch.from_numpy(win.field).cuda())
    ws = engine.Workspace()
    full = torch.empty((n, 3, size, size), dtype=torch.float16, device=rgb.device)
    w64 = torch.from_numpy(win.affine.astype(np.float64) / Q).cuda()
    cy, cx, a00, a01, a10, a11 = (w64[:, k] for k in range(6))
    theta = torch.stack([torch.stack([a11 * crop / size, a10 * crop / size, 2 * cx / size - 1], dim=1),
                         torch.stack([a01 * crop / size, a00 * crop / size, 2 * cy / size - 1], dim=1)], dim=1).to(torch.float16)
    # the control lattice as grid_sample's normalised (x, y) offsets: 1/256 source pixel -> 2 / size
    lat = (dwin.field.to(torch.float16) * (2.0 / (256.0 * size))).flip(-1).permute(0, 3, 1, 2).contiguous()

    def dense_grid(dtype):
        grid = torch.nn.functional.affine_grid(theta.to(dtype), (n, 3, crop, crop), align_corners=False)
        return grid + torch.nn.functional.interpolate(lat.to(dtype), size=(crop, crop), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)

    def fused_host():
        return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=win)[0]

    def fused_dev():
        return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]

    def chain():
        x = nz.augment_batch(rgb, ab, out=full, ws=ws, tensor_format=f16)[0]
        return torch.nn.functional.grid_sample(x, dense_grid(torch.float16), mode="bilinear", padding_mode="zeros", align_corners=False)

    assert torch.equal(fused_host().view(torch.int16).clone(), fused_dev().view(torch.int16))
    tc, th, td = timed(chain), timed(fused_host), timed(fused_dev)
    lines += ["", "(b) augment_batch, fits included; %d tiles of %d^2, %r -> float16 NCHW" % (n, size, view),
              row("chain: augment_batch(tensor_format=) -> affine_grid + upsampled lattice -> grid_sample(bilinear, zeros)", tc),
              row("fused: augment_batch(view=, tensor_format=), windows on the host (launch sized by their own bounds)", th),
              row("fused: the same, windows on the device (launch sized by the view's bound and max_d)", td),
              "    the fused call takes %.2f (host windows) and %.2f (device windows) of the chain's time (the chain is another definition: "
              "see the tool's docstring)" % (th[0] / tc[0], td[0] / tc[0])]
    del full
    torch.cuda.empty_cache()

    # ---- (c) int64 labels
    labels = torch.randint(0, 6, (n, size // 8, size // 8), device=rgb.device, dtype=torch.int64)
    labels = labels.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).contiguous()        # blobs of 8 x 8
    lout = torch.empty((n, crop, crop), dtype=torch.int64, device=rgb.device)

    def planes_fused():
        return view.apply(labels, dwin, fill=255, out=lout)

    def planes_chain():
        return torch.nn.functional.grid_sample(labels[:, None].float(), dense_grid(torch.float32), mode="nearest", padding_mode="zeros",
                                               align_corners=False)[:, 0].long()

    tpc, tpf = timed(planes_chain), timed(planes_fused)
    lines += ["", "(c) int64 labels, %d planes of %d^2 -> %d^2, the windows of (b) on the device" % (n, size, crop),
              row("chain: float32 copy -> affine_grid + upsampled lattice -> grid_sample(mode='nearest') -> int64", tpc),
              row("fused: TileElastic.apply (sl_view_planes_elastic, 8-byte elements)", tpf),
              "    the fused call takes %.2f of the chain's time" % (tpf[0] / tpc[0])]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

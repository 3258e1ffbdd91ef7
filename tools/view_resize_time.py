"""What the resizing view (random-resized crop inside the view pass) costs: its write side beside the fixed-size views on
the same windows, and the whole call beside the chain it replaces, full-tile tensor -> per-tile slice -> interpolate(mode="area").
    python tools/view_resize_time.py [--out profiles/view_resize_time.txt] [--tiles 512] [--size 1024] [--collections 5]
Device-resident synthetic tiles, 512 tiles of 1024^2 -> 224^2, float16 NCHW, mixed codes.  Timed by HIP events after a 0.25 s spin-up of
the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections (their min
and max beside it).  Every yardstick is existing code, timed in the same process as what it is compared with:
  (a) the write side: sl_normalize_view_resize (the jitter route) with 224^2 windows beside sl_normalize_view on the same windows, and
      with 448^2 windows beside sl_normalize_view_shrink at s = 2 -- the same reads and per-source-pixel arithmetic, so the difference
      is the geometry and the write side
  (b) end to end, fits included, TileView(224, scale=(0.08, 1)): augment_batch(view=, tensor_format=) against augment_batch(
      tensor_format=) on the full tile followed by the loop a loader runs today: per tile slice, interpolate(mode="area"), flip, rot90
  (c) sl_normalize_view at shrink = 1 on the shapes of tools/view_time.py: the figure to put beside an earlier build's
(The chain of (b) is ANOTHER definition: interpolate(mode="area") is adaptive average pooling -- whole source pixels, equal weights -- on
float16 values; the fused pass weights source pixels by their overlap and averages bytes.  They are not compared bit for bit; the largest
difference is printed.)
Each step runs in a process of its own under `timeout`; a step that ends with a non-zero status ends the run, and nothing further is
started on the device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

STEPS = ("a", "b", "c")


def step(args):
    sys.path.insert(0, ".")
    import numpy as np
    import torch
    import stainlib_amd
    from stainlib_amd import engine
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
        return "  %-100s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])

    target = synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy()
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    n, size, crop = args.tiles, args.size, 224
    lines = []

    def jitter_setup(n, size):
        nz = stainlib_amd.MacenkoNormalizer()
        nz.fit(target)
        rgb = synth_tiles(n, size, size, seed=9)
        M, maxC, status = engine.macenko_fit(rgb)
        assert int((status != 0).sum()) == 0
        Mt, ct = nz._target_on(rgb.device)
        np.random.seed(3)
        ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=rgb.device)
        return nz, rgb, (M, maxC, Mt, ct, ab)

    if args.step == "a":
        nz, rgb, route = jitter_setup(n, size)
        out = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=rgb.device)
        lines.append("(a) %d tiles of %d^2 -> %d^2, jitter route -> float16 NCHW, all eight codes" % (n, size, crop))
        for s in (1, 2):
            np.random.seed(4)
            win3 = stainlib_amd.TileView(crop, shrink=s).draw(n, size, size)
            win5 = np.concatenate([win3, np.full((n, 2), s * crop, dtype=np.int32)], axis=1)
            d3, d5 = torch.from_numpy(win3).cuda(), torch.from_numpy(win5).cuda()
            t0 = timed(lambda: engine.normalize_view(rgb, d3, crop, 7, *route, fmt=f16, out=out, shrink=s))
            want = out.clone()
            t1 = timed(lambda: engine.normalize_view(rgb, d5, crop, 7, *route, fmt=f16, out=out, resize=(s * crop, s * crop)))
            assert torch.equal(out.view(torch.int16), want.view(torch.int16))
            lines.append(row("sl_normalize_view%s on %d^2 windows" % ("" if s == 1 else "_shrink, s = %d," % s, s * crop), t0))
            lines.append(row("sl_normalize_view_resize on the same windows (same bits)", t1))
            lines.append("    the resizing view takes %.2f of the fixed-size view's time" % (t1[0] / t0[0]))
    elif args.step == "b":
        nz, rgb, route = jitter_setup(n, size)
        ab = route[4]
        ws = engine.Workspace()
        view = stainlib_amd.TileView(crop, scale=(0.08, 1))
        np.random.seed(4)
        win = view.draw(n, size, size)
        dwin = torch.from_numpy(win).cuda()
        out = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=rgb.device)
        full = torch.empty((n, 3, size, size), dtype=torch.float16, device=rgb.device)
        rows = win.tolist()

        def fused_host():
            return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=win)[0]

        def fused_dev():
            return nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]

        def chain():
            x = nz.augment_batch(rgb, ab, out=full, ws=ws, tensor_format=f16)[0]
            res = torch.empty_like(out)
            for t, (y0, x0, d, wh, ww) in enumerate(rows):
                nu, nv = (crop, crop)
                v = torch.nn.functional.interpolate(x[t:t + 1, :, y0:y0 + wh, x0:x0 + ww], size=(nu, nv), mode="area")[0]
                if d & 4:
                    v = torch.flip(v, dims=(2,))
                res[t] = torch.rot90(v, d & 3, dims=(1, 2))
            return res

        diff = float((chain().float() - fused_host().float()).abs().max())
        assert torch.equal(fused_host().view(torch.int16).clone(), fused_dev().view(torch.int16))
        tc, th, td = timed(chain), timed(fused_host), timed(fused_dev)
        area = win[:, 3].astype(np.int64) * win[:, 4]
        lines.append("(b) augment_batch, fits included; %d tiles of %d^2, TileView(%d, scale=(0.08, 1)): windows of %d..%d px a side, mean share "
                     "of the tile %.2f -> float16 NCHW" % (n, size, crop, int(win[:, 3:].min()), int(win[:, 3:].max()),
                                                          float(area.mean()) / (size * size)))
        lines.append(row("chain: augment_batch(tensor_format=) -> per tile slice, interpolate(mode='area'), flip, rot90", tc))
        lines.append(row("fused: augment_batch(view=, tensor_format=), windows on the host (launch sized by their largest sides)", th))
        lines.append(row("fused: the same, windows on the device (launch sized by the view's bound, the whole tile)", td))
        lines.append("    the fused call takes %.2f (host windows) and %.2f (device windows) of the chain's time; largest |chain - fused| = %.4f "
                     "(another definition: see the tool's docstring)" % (th[0] / tc[0], td[0] / tc[0], diff))
    else:
        lines.append("(c) sl_normalize_view at shrink = 1 (jitter route -> float16 NCHW) on the shapes of tools/view_time.py")
        for n2, size2, crop2 in ((512, 1024, 896), (4096, 256, 224)):
            nz, rgb, route = jitter_setup(n2, size2)
            np.random.seed(4)
            dwin = torch.from_numpy(stainlib_amd.TileView(crop2).draw(n2, size2, size2)).cuda()
            out = torch.empty((n2, 3, crop2, crop2), dtype=torch.float16, device=rgb.device)
            lines.append(row("sl_normalize_view %d x %d^2 -> %d^2" % (n2, size2, crop2),
                             timed(lambda: engine.normalize_view(rgb, dwin, crop2, 7, *route, fmt=f16, out=out))))
            del rgb, out, nz, route
            torch.cuda.empty_cache()
    head = "device %s; " % torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        f.write(head + "\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/view_resize_time.txt")
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--collections", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each step's process may take")
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process and write its lines to --part")
    ap.add_argument("--part")
    args = ap.parse_args()
    if args.step:
        return step(args)
    text = ["ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up; one process per "
            "step" % args.collections]
    rc = 0
    for name in STEPS:
        part = "%s.%s.part" % (args.out, name)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--part", part,
               "--tiles", str(args.tiles), "--size", str(args.size), "--collections", str(args.collections)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                               # a fault, an abort or the time limit: nothing further on the device
            text += ["", "(%s) ended with status %d: not measured, and the steps behind it were not started" % (name, rc)]
            break
        body = open(part).read().splitlines()
        os.remove(part)
        if len(text) == 1:
            text[0] = body[0] + text[0]
        text += [""] + body[1:]
    out = "\n".join(text) + "\n"
    print(out, flush=True)
    with open(args.out, "w") as f:
        f.write(out)
    return rc


if __name__ == "__main__":
    sys.exit(main())

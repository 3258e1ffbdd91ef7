"""What the stain jitter inside the apply pass costs, beside k_apply and beside the chain a loader ran before it existed.
    python tools/jitter_time.py [--out profiles/jitter_time.txt] [--shapes 512x1024] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko) for the passes that take statistics.  Per shape, timed by HIP events after a
0.25 s spin-up of the same call (the clocks ramp for ~25 ms); a COLLECTION is the median of 20 single launches, and the figure in the
file is the median of the collections (their min and max beside it), with the achieved TB/s at the bytes the algorithm moves:
  0. k_apply alone (sl_normalize_apply): 3 + 3 B/px -- the yardstick of the new pass
  1. sl_normalize_jitter to uint8, tissue only and all pixels: 3 + 3 B/px
  2. sl_normalize_jitter to the model-ready tensor, float16 NCHW: 3 + 6 B/px; float32 NCHW: 3 + 12 B/px
  3. today's chain to the same float16 tensor: transform_batch -> macenko_fit of the NORMALISED tiles -> stain_augment -> convert
  4. the new route to it: macenko_fit -> sl_normalize_jitter (what augment_batch(tensor_format=) runs)
The chain perturbs under the re-fitted matrix of the normalised tiles, the new pass under the target's: they agree to the fit's error,
not byte for byte, so nothing is compared here (tests/test_gpu_jitter.py holds the pass to its neighbours and to the oracle)."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/jitter_time.txt")
    ap.add_argument("--shapes", default="512x1024")
    ap.add_argument("--collections", type=int, default=5)
    args = ap.parse_args()
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

    def row(label, t, bytes_moved=None):
        tail = "   %.2f TB/s" % (bytes_moved / (t[0] * 1e-3) / 1e12) if bytes_moved else ""
        return "  %-78s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    f32 = stainlib_amd.TensorFormat(dtype=torch.float32, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    lines = ["device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up"
             % (torch.cuda.get_device_name(0), args.collections)]
    for shape in args.shapes.split(","):
        n, size = (int(x) for x in shape.split("x"))
        px = n * size * size
        rgb = synth_tiles(n, size, size, seed=9)
        M, maxC, status = engine.macenko_fit(rgb)
        assert int((status != 0).sum()) == 0
        Mt, ct = nz._target_on(rgb.device)
        np.random.seed(3)
        ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=rgb.device)
        u8, u8b = torch.empty_like(rgb), torch.empty_like(rgb)
        t16 = torch.empty((n, 3, size, size), dtype=torch.float16, device=rgb.device)
        t32 = torch.empty((n, 3, size, size), dtype=torch.float32, device=rgb.device)
        ws = engine.Workspace()
        lines += ["", "%d tiles of %d^2 (%.1f Mpx)" % (n, size, px / 1e6)]

        def chain():
            a, _, _, _ = nz.transform_batch(rgb, out=u8, ws=ws)
            M2, _, _ = engine.macenko_fit(a, ws=ws)
            b = engine.stain_augment(a, M2, ab, out=u8b)
            return f16.convert(b, out=t16)

        def route():
            M1, c1, _ = engine.macenko_fit(rgb, ws=ws)
            return engine.normalize_jitter(rgb, M1, c1, Mt, ct, ab, fmt=f16, out=t16)

        lines.append(row("0. k_apply alone (sl_normalize_apply), 6 B/px", timed(lambda: engine.normalize_apply(rgb, M, maxC, Mt, ct, out=u8)), 6 * px))
        lines.append(row("1. sl_normalize_jitter -> uint8, tissue only, 6 B/px",
                         timed(lambda: engine.normalize_jitter(rgb, M, maxC, Mt, ct, ab, out=u8)), 6 * px))
        lines.append(row("   sl_normalize_jitter -> uint8, all pixels, 6 B/px",
                         timed(lambda: engine.normalize_jitter(rgb, M, maxC, Mt, ct, ab, augment_background=True, out=u8)), 6 * px))
        lines.append(row("2. sl_normalize_jitter -> float16 NCHW, tissue only, 9 B/px",
                         timed(lambda: engine.normalize_jitter(rgb, M, maxC, Mt, ct, ab, fmt=f16, out=t16)), 9 * px))
        lines.append(row("   sl_normalize_jitter -> float32 NCHW, tissue only, 15 B/px",
                         timed(lambda: engine.normalize_jitter(rgb, M, maxC, Mt, ct, ab, fmt=f32, out=t32)), 15 * px))
        lines.append(row("3. chain: transform_batch -> macenko_fit -> stain_augment -> convert (float16 NCHW)", timed(chain)))
        lines.append(row("4. new route: macenko_fit -> sl_normalize_jitter (float16 NCHW)", timed(route)))
        del rgb, u8, u8b, t16, t32, ws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

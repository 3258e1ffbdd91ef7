"""What the stain separation costs, beside the chain a caller composed before it existed.
    python tools/separate_time.py [--out profiles/separate_time.txt] [--shapes 512x1024,1250x512]
Device-resident synthetic tiles, fitted once (Macenko); the apply-side passes alone are timed.  Every figure is the median of 20
launches timed one by one with HIP events after a 0.25 s spin-up of the same call (min and max beside it), with the achieved TB/s at
the bytes the algorithm moves.  Timed:
  0. k_apply alone (sl_normalize_apply): 3 + 3 B/px
  1. sl_stain_separate, all four outputs, float32 planes: 3 + 9 + 8 = 20 B/px; float16 planes: 3 + 9 + 4 = 16 B/px
  2. sl_stain_separate, the two stain images only: 3 + 6 B/px
  3. sl_stain_separate, the planes only: 3 + 8 B/px (float32), 3 + 4 B/px (float16)
  4. the chain: three sl_normalize_apply calls (full target, E row zeroed, H row zeroed) plus sl_concentrations -- 4 x 3 B/px read,
     9 + 8 B/px written; its planes are raw, interleaved float32 (not rescaled, not planar)
and the outputs of 1 are compared with the chain's images (torch.equal) before anything is timed."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/separate_time.txt")
    ap.add_argument("--shapes", default="512x1024,1250x512")
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import torch
    from stainlib_amd import engine
    from tools.synth import synth_tiles

    def timed(fn, reps=20):
        """(median, min, max) ms of `reps` calls timed one by one, after a spin-up (the clocks ramp for ~25 ms)"""
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
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        return statistics.median(ms), min(ms), max(ms)

    def row(label, t, bytes_moved):
        return "  %-62s %8.3f ms  (min %.3f, max %.3f)   %.2f TB/s" % (label, t[0], t[1], t[2], bytes_moved / (t[0] * 1e-3) / 1e12)

    Mt, ct, st = engine.macenko_fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]]))
    assert int(st[0]) == 0
    Mt, ct = Mt[0].contiguous(), ct[0].contiguous()
    only_h, only_e = Mt.clone(), Mt.clone()
    only_h[1] = 0.0
    only_e[0] = 0.0
    lines = ["device %s; ms per call, median of 20 single launches by HIP events after a 0.25 s spin-up" % torch.cuda.get_device_name(0)]
    for shape in args.shapes.split(","):
        n, size = (int(x) for x in shape.split("x"))
        px = n * size * size
        rgb = synth_tiles(n, size, size, seed=9)
        M, maxC, status = engine.macenko_fit(rgb)
        assert int((status != 0).sum()) == 0
        S = engine.Separated
        u8 = [torch.empty_like(rgb) for _ in range(3)]
        c32 = torch.empty((n, 2, size, size), dtype=torch.float32, device=rgb.device)
        c16 = torch.empty((n, 2, size, size), dtype=torch.float16, device=rgb.device)
        lines += ["", "%d tiles of %d^2 (%.1f Mpx)" % (n, size, px / 1e6)]

        def chain():
            a = engine.normalize_apply(rgb, M, maxC, Mt, ct, out=u8[0])
            b = engine.normalize_apply(rgb, M, maxC, only_h, ct, out=u8[1])
            c = engine.normalize_apply(rgb, M, maxC, only_e, ct, out=u8[2])
            return a, b, c, engine.concentrations(rgb, M)

        # faster and different is not faster: the same images first
        sep = engine.stain_separate(rgb, M, maxC, Mt, ct)
        a, b, c, raw = chain()
        assert torch.equal(sep.norm, a) and torch.equal(sep.h, b) and torch.equal(sep.e, c)
        del sep, a, b, c, raw
        torch.cuda.empty_cache()

        lines.append(row("0. k_apply alone (sl_normalize_apply), 6 B/px", timed(lambda: engine.normalize_apply(rgb, M, maxC, Mt, ct, out=u8[0])), 6 * px))
        full32 = S(u8[0], u8[1], u8[2], c32)
        lines.append(row("1. separate: norm + h + e + conc float32, 20 B/px",
                         timed(lambda: engine.stain_separate(rgb, M, maxC, Mt, ct, out=full32)), 20 * px))
        full16 = S(u8[0], u8[1], u8[2], c16)
        lines.append(row("   separate: norm + h + e + conc float16, 16 B/px",
                         timed(lambda: engine.stain_separate(rgb, M, maxC, Mt, ct, conc_dtype=torch.float16, out=full16)), 16 * px))
        he = S(h=u8[1], e=u8[2])
        lines.append(row("2. separate: h + e, 9 B/px", timed(lambda: engine.stain_separate(rgb, M, maxC, Mt, ct, want=("h", "e"), out=he)), 9 * px))
        lines.append(row("3. separate: conc float32, 11 B/px",
                         timed(lambda: engine.stain_separate(rgb, M, maxC, Mt, ct, want=("conc",), out=S(conc=c32))), 11 * px))
        lines.append(row("   separate: conc float16, 7 B/px",
                         timed(lambda: engine.stain_separate(rgb, M, maxC, Mt, ct, want=("conc",), conc_dtype=torch.float16, out=S(conc=c16))), 7 * px))
        t_chain = timed(chain)
        lines.append(row("4. chain: 3 x sl_normalize_apply + sl_concentrations, 29 B/px", t_chain, 29 * px))
        del rgb, u8, c32, c16, full32, full16, he
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

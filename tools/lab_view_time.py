"""What the Reinhard map costs fused with the view (crop, flip, quarter turn) and the tensor conversion, beside the two-kernel tail it
replaces.
    python tools/lab_view_time.py [--out profiles/lab_view_time.txt] [--shapes 1250x512:448,512x1024:896] [--collections 5]
Device-resident synthetic tiles, a target fitted once.  Per shape (n tiles of size^2 -> crop^2), timed by HIP events after a 0.25 s
spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections
(their min and max beside it).  Mixed codes and corners from TileView.draw, mask_background on, float16 NCHW out.  Every yardstick is
existing code, timed in the same process:
  (a) the map alone: k_lab_view against the tail it replaces, k_lab_map<0> then convert(view=) on the same windows.  Neither has an
      entry point of its own, so each is a whole call minus the statistics both share: reinhard_stats (the two histogram sweeps and the
      per-tile numbers) is timed beside them and subtracted; what stays on both sides is the one-workgroup-per-tile table kernel.
      B/s: the fused map at 3 B read + 6 B written per WINDOW pixel; the tail at 3 + 3 B per tile pixel plus 3 + 6 B per window pixel.
  (b) the whole call: transform_batch(view=, tensor_format=) against transform_batch() -> convert(view=), statistics included.
The two results agree bit for bit (checked once per shape before timing)."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lab_view_time.txt")
    ap.add_argument("--shapes", default="1250x512:448,512x1024:896")
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

    def row(label, t):
        return "  %-92s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])

    nz = stainlib_amd.ReinhardStainNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    lines = ["device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up"
             % (torch.cuda.get_device_name(0), args.collections)]
    for shape in args.shapes.split(","):
        n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
        wpx, tpx = n * crop * crop, n * size * size
        rgb = synth_tiles(n, size, size, seed=9)
        dev = rgb.device
        view = stainlib_amd.TileView(crop)
        np.random.seed(3)
        win = view.draw(n, size, size)
        dwin = torch.from_numpy(win).to(dev)
        u8 = torch.empty_like(rgb)
        t16c = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
        t16v = torch.empty_like(t16c)
        ws = engine.Workspace()

        def chain():
            full, _ = nz.transform_batch(rgb, mask_background=True, out=u8, ws=ws)
            return f16.convert(full, out=t16c, view=view, windows=dwin)[0]

        def fused():
            return nz.transform_batch(rgb, mask_background=True, out=t16v, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]

        assert torch.equal(chain().view(torch.int16), fused().view(torch.int16)), "the chain and the fused pass disagree"
        lines += ["", "%d tiles of %d^2 -> %d^2 (%.1f Mpx written of %.1f: %.0f %% discarded), codes %s" % (
            n, size, crop, wpx / 1e6, tpx / 1e6, 100.0 * (1 - wpx / tpx), sorted(set(win[:, 2].tolist())))]
        ts = timed(lambda: engine.reinhard_stats(rgb, ws=ws))
        tc, tf = timed(chain), timed(fused)
        map_c, map_f = tc[0] - ts[0], tf[0] - ts[0]
        bytes_c, bytes_f = 6 * tpx + 9 * wpx, 9 * wpx
        lines.append(row("shared: reinhard_stats (both histogram sweeps and the per-tile numbers)", ts))
        lines.append(row("(b) chain: transform_batch() -> convert(view=), float16 NCHW", tc))
        lines.append(row("(b) fused: transform_batch(view=, tensor_format=)", tf))
        lines.append("    the fused call takes %.2f of the chain's time%s" % (tf[0] / tc[0], "" if tf[0] < tc[0] else
                                                                             "  -- the fused pass is not faster at this shape"))
        lines.append("  (a) the map alone, (b) minus the shared statistics:")
        lines.append("    tail: k_lab_map<0> + convert(view=)   %8.3f ms   %.2f TB/s at %d B per tile px + %d B per window px"
                     % (map_c, bytes_c / (map_c * 1e-3) / 1e12, 6, 9))
        lines.append("    k_lab_view                            %8.3f ms   %.2f TB/s at %d B per window px" % (map_f, bytes_f / (map_f * 1e-3) / 1e12, 9))
        lines.append("    k_lab_view takes %.2f of the tail's time%s" % (map_f / map_c, "" if map_f < map_c else
                                                                       "  -- the fused pass is not faster at this shape"))
        del rgb, u8, t16c, t16v, ws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""What the companion planes of a view pass cost (sl_view_planes, TileView.apply), beside a plain copy of as many bytes, beside the
existing image kernel on the same windows and beside the chain the call replaces.
    python tools/planes_view_time.py [--out profiles/planes_view_time.txt] [--collections 5]
Device-resident planes of arbitrary bits, mixed codes and corners from TileView.draw.  Timed by HIP events after a 0.25 s spin-up of the
same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections (their min and
max beside it); everything in one process, every line printed and written as soon as it is measured (the whole takes about 15 minutes).  Shapes: 512 planes of 1024^2 -> 896^2 and 4096 planes of 256^2 -> 224^2.
Every yardstick is existing code, never the new call against itself:
  (a) sl_view_planes, nearest, at 1, 2, 4 and 8 bytes per element, beside a device-to-device copy_ of as many bytes as the call reads
      and writes (the windows' elements twice); for uint8 with c = 3 beside sl_normalize_view on its raw route on the same windows and
      the same bytes as (N, H, W, 3) images.  Bytes per second for each.
  (b) the same at shrink = 2 and under scale = (0.08, 1) windows (uint8 and int64, nearest; uint8 area beside the image kernel)
  (c) against the chain it replaces: the per-tile torch slice / index / flip / rot90 loop on the same windows, same bits (int64 labels)"""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/planes_view_time.txt")
    ap.add_argument("--collections", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import numpy as np
    import torch
    import stainlib_amd
    from stainlib_amd import engine

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

    def row(label, t, nbytes=None):
        tail = "" if nbytes is None else "  %8.1f GB/s" % (nbytes / (t[0] * 1e-3) / 1e9)
        return "  %-96s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

    class Lines(list):                                               # every line is printed and written as it is measured
        def append(self, s):
            print(s, flush=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")
            super().append(s)

    open(args.out, "w").close()
    lines = Lines()
    lines.append("device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up; "
                 "one process.  GB/s: bytes read plus bytes written (the windows' elements, and the outputs) per second"
                 % (torch.cuda.get_device_name(0), args.collections))

    def planes(n, size, es, c=None):
        shape = (n, size, size) if c is None else (n, c, size, size)
        return torch.randint(0, 256, (int(np.prod(shape)) * es,), dtype=torch.uint8, device="cuda").view(INT[es]).view(shape)

    def draw(view, n, size):
        np.random.seed(4)
        win = view.draw(n, size, size)
        return win, torch.from_numpy(win).cuda()

    def read_elems(win, oh, ow, s):
        """elements of the windows of one plane each"""
        if win.shape[1] == 5:
            return int((win[:, 3].astype(np.int64) * win[:, 4]).sum())
        return win.shape[0] * s * s * oh * ow

    def copy_row(nbytes_moved):
        src = torch.empty((nbytes_moved // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src))
        return row("    copy_ of %d bytes device to device (as many read, as many written)" % src.numel(), t, 2 * src.numel())

    for nplanes, size, crop in ((512, 1024, 896), (4096, 256, 224)):
        lines.append("")
        lines.append("==== %d planes of %d^2 -> %d^2" % (nplanes, size, crop))
        # (a) crop / flip / turn
        view = stainlib_amd.TileView(crop)
        win, dwin = draw(view, nplanes, size)
        lines.append("(a) sl_view_planes, nearest, crop / flip / turn; codes %s" % sorted(set(win[:, 2].tolist())))
        for es in (1, 2, 4, 8):
            x = planes(nplanes, size, es)
            out = torch.empty((nplanes, crop, crop), dtype=x.dtype, device="cuda")
            moved = 2 * nplanes * crop * crop * es
            lines.append(row("sl_view_planes %d B / element" % es, timed(lambda: engine.view_planes(x, dwin, crop, out=out)), moved))
            lines.append(copy_row(moved))
            del x, out
            torch.cuda.empty_cache()
        n3 = nplanes // 3
        x = planes(n3, size, 1, c=3)
        img = x.permute(0, 2, 3, 1).contiguous()
        win3, dwin3 = draw(view, n3, size)
        out = torch.empty((n3, 3, crop, crop), dtype=torch.uint8, device="cuda")
        oimg = torch.empty((n3, crop, crop, 3), dtype=torch.uint8, device="cuda")
        moved = 2 * n3 * 3 * crop * crop
        assert torch.equal(engine.view_planes(x, dwin3, crop, out=out), engine.normalize_view(img, dwin3, crop, out=oimg).permute(0, 3, 1, 2))
        lines.append(row("sl_view_planes uint8, c = 3 (%d tiles)" % n3, timed(lambda: engine.view_planes(x, dwin3, crop, out=out)), moved))
        lines.append(row("sl_normalize_view, raw route, the same bytes as (N, H, W, 3) images, same windows",
                         timed(lambda: engine.normalize_view(img, dwin3, crop, out=oimg)), moved))
        # (b) shrink = 2 and scale = (0.08, 1)
        small = crop // 2
        lines.append("(b) shrink = 2 (%d^2 windows -> %d^2) and scale = (0.08, 1) windows -> %d^2" % (crop, small, crop))
        v2 = stainlib_amd.TileView(small, shrink=2)
        w2, dw2 = draw(v2, n3, size)
        vs = stainlib_amd.TileView(crop, scale=(0.08, 1))
        ws_, dws = draw(vs, n3, size)
        bound = vs.window_bound(size, size)
        o2 = torch.empty((n3, 3, small, small), dtype=torch.uint8, device="cuda")
        oi2 = torch.empty((n3, small, small, 3), dtype=torch.uint8, device="cuda")
        rd2, rds = 3 * read_elems(w2, small, small, 2), 3 * read_elems(ws_, crop, crop, 1)
        for mode in ("nearest", "area"):
            lines.append(row("sl_view_planes uint8 c = 3, shrink = 2, %s" % mode,
                             timed(lambda: engine.view_planes(x, dw2, small, out=o2, shrink=2, mode=mode)), rd2 + o2.numel()))
        assert torch.equal(o2, engine.normalize_view(img, dw2, small, out=oi2, shrink=2).permute(0, 3, 1, 2))
        lines.append(row("sl_normalize_view_shrink, raw route, same bytes, same windows",
                         timed(lambda: engine.normalize_view(img, dw2, small, out=oi2, shrink=2)), rd2 + oi2.numel()))
        lines.append(copy_row(rd2 + o2.numel()))
        for mode in ("nearest", "area"):
            lines.append(row("sl_view_planes uint8 c = 3, scale = (0.08, 1), %s" % mode,
                             timed(lambda: engine.view_planes(x, dws, crop, out=out, resize=bound, mode=mode)), rds + out.numel()))
        assert torch.equal(out, engine.normalize_view(img, dws, crop, out=oimg, resize=bound).permute(0, 3, 1, 2))
        lines.append(row("sl_normalize_view_resize, raw route, same bytes, same windows",
                         timed(lambda: engine.normalize_view(img, dws, crop, out=oimg, resize=bound)), rds + oimg.numel()))
        lines.append(copy_row(rds + out.numel()))
        del x, img, out, oimg, o2, oi2
        torch.cuda.empty_cache()
        x = planes(nplanes, size, 8)
        w2, dw2 = draw(v2, nplanes, size)
        ws_, dws = draw(vs, nplanes, size)
        o2 = torch.empty((nplanes, small, small), dtype=torch.int64, device="cuda")
        out = torch.empty((nplanes, crop, crop), dtype=torch.int64, device="cuda")
        lines.append(row("sl_view_planes int64, shrink = 2, nearest", timed(lambda: engine.view_planes(x, dw2, small, out=o2, shrink=2)),
                         8 * (read_elems(w2, small, small, 2) + o2.numel())))
        lines.append(row("sl_view_planes int64, scale = (0.08, 1), nearest", timed(lambda: engine.view_planes(x, dws, crop, out=out, resize=bound)),
                         8 * (read_elems(ws_, crop, crop, 1) + out.numel())))
        # (c) the chain it replaces, on int64 labels
        lines.append("(c) int64 labels: TileView.apply against the per-tile torch slice / index / flip / rot90 loop on the same windows")

        def chain(win, oh, ow, s, dst):
            for t, r in enumerate(win.tolist()):
                y0, x0, d = r[:3]
                nu, nv = (ow, oh) if d & 1 else (oh, ow)
                wh, ww = (r[3], r[4]) if len(r) == 5 else (s * nu, s * nv)
                v = x[t, y0:y0 + wh, x0:x0 + ww]
                if (wh, ww) != (nu, nv):
                    ky = ((2 * torch.arange(nu, device="cuda") + 1) * wh) // (2 * nu)
                    kx = ((2 * torch.arange(nv, device="cuda") + 1) * ww) // (2 * nv)
                    v = v[ky][:, kx]
                if d & 4:
                    v = torch.flip(v, dims=(1,))
                dst[t] = torch.rot90(v, d & 3, dims=(0, 1))
            return dst

        for label, v, w_host, w_dev, dst in (("crop", view, win, dwin, out), ("shrink = 2", v2, w2, dw2, o2), ("scale = (0.08, 1)", vs, ws_, dws, out)):
            oh = ow = dst.shape[-1]
            want = chain(w_host, oh, ow, v.shrink, torch.empty_like(dst))
            same = torch.equal(v.apply(x, w_dev), want)
            tc = timed(lambda: chain(w_host, oh, ow, v.shrink, dst))
            tf = timed(lambda: v.apply(x, w_dev, out=dst))
            lines.append(row("%s: torch loop per tile" % label, tc))
            lines.append(row("%s: TileView.apply (same bits: %s)" % (label, same), tf))
            lines.append("    apply takes %.3f of the loop's time%s" % (tf[0] / tc[0], "" if tf[0] < tc[0] else "  -- apply is NOT faster at this shape"))
        del x, out, o2
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())

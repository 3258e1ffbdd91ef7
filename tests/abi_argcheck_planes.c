/* Argument checks of the companion-planes entry point of the C ABI (include/stainlib_hip.h: sl_view_planes) on the HOST side, no GPU
 * needed: every refused call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under AddressSanitizer
 * by `make -C stainlib_amd/csrc asan-planes` (tests/test_planes_view_host.py).  The data pointers are DEVICE pointers the host side never
 * reads through: the non-null ones below are deliberately wild -- the windows too, which are clamped on the device and never read back. */
#include "abi_argcheck.h"

int main(void) {
    void* pl = (void*)0x100000;
    void* out = (void*)0x200000;
    int32_t* win = (int32_t*)0x300300;
    const int n = 4, c = 3, h = 64, w = 48;
    EXPECT(sl_version(), SL_VERSION);

/* a crop / shrink call and a resizing call */
#define CR(pl_, out_, n_, c_, h_, w_, eb_, oh_, ow_, win_, dm_, s_, mode_) \
        EXPECT(sl_view_planes(pl_, out_, n_, c_, h_, w_, eb_, oh_, ow_, win_, dm_, s_, 0, 0, mode_, 0), SL_ERR_BADARG)
#define RS(pl_, out_, n_, c_, h_, w_, eb_, oh_, ow_, win_, dm_, s_, mh_, mw_, mode_) \
        EXPECT(sl_view_planes(pl_, out_, n_, c_, h_, w_, eb_, oh_, ow_, win_, dm_, s_, mh_, mw_, mode_, 0), SL_ERR_BADARG)
/* both, at every element size and (uint8) in both modes */
#define ALL(pl_, out_, n_, c_, h_, w_, oh_, ow_, win_, dm_) do { \
        const int eb_[] = {1, 2, 4, 8}; \
        for (int i_ = 0; i_ < 4; ++i_) { \
            CR(pl_, out_, n_, c_, h_, w_, eb_[i_], oh_, ow_, win_, dm_, 1, SL_PLANES_NEAREST); \
            RS(pl_, out_, n_, c_, h_, w_, eb_[i_], oh_, ow_, win_, dm_, 1, 8, 8, SL_PLANES_NEAREST); } \
        CR(pl_, out_, n_, c_, h_, w_, 1, oh_, ow_, win_, dm_, 1, SL_PLANES_AREA); \
        RS(pl_, out_, n_, c_, h_, w_, 1, oh_, ow_, win_, dm_, 1, 8, 8, SL_PLANES_AREA); } while (0)

    /* NULL pointers */
    ALL(0, out, n, c, h, w, 8, 8, win, 7);
    ALL(pl, 0, n, c, h, w, 8, 8, win, 7);
    ALL(pl, out, n, c, h, w, 8, 8, 0, 7);
    /* n, c, h, w, oh, ow <= 0 */
    {
        const int bad[] = {0, -1, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            ALL(pl, out, bad[i], c, h, w, 8, 8, win, 7);
            ALL(pl, out, n, bad[i], h, w, 8, 8, win, 7);
            ALL(pl, out, n, c, bad[i], w, 8, 8, win, 7);
            ALL(pl, out, n, c, h, bad[i], 8, 8, win, 7);
            ALL(pl, out, n, c, h, w, bad[i], 8, win, 7);
            ALL(pl, out, n, c, h, w, 8, bad[i], win, 7);
        }
    }
    /* h w > 2^30 (the product overflows an int: refused, not wrapped) */
    ALL(pl, out, n, c, 32768, 32769, 8, 8, win, 7);
    ALL(pl, out, n, c, 65536, 65536, 8, 8, win, 7);
    /* elem_bytes */
    {
        const int bad[] = {0, -1, 3, 5, 6, 7, 9, 16, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            CR(pl, out, n, c, h, w, bad[i], 8, 8, win, 7, 1, SL_PLANES_NEAREST);
            RS(pl, out, n, c, h, w, bad[i], 8, 8, win, 7, 1, 8, 8, SL_PLANES_NEAREST);
        }
    }
    /* planes or out not aligned to elem_bytes */
    {
        const int eb[] = {2, 4, 8};
        for (int i = 0; i < 3; ++i)
            for (int off = 1; off < eb[i]; ++off) {
                CR((char*)pl + off, out, n, c, h, w, eb[i], 8, 8, win, 7, 1, SL_PLANES_NEAREST);
                CR(pl, (char*)out + off, n, c, h, w, eb[i], 8, 8, win, 7, 1, SL_PLANES_NEAREST);
                RS((char*)pl + off, out, n, c, h, w, eb[i], 8, 8, win, 7, 1, 8, 8, SL_PLANES_NEAREST);
                RS(pl, (char*)out + off, n, c, h, w, eb[i], 8, 8, win, 7, 1, 8, 8, SL_PLANES_NEAREST);
            }
    }
    /* an unknown mode; the area mode on anything but one byte */
    {
        const int bad[] = {2, -1, 99, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            CR(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, bad[i]);
            CR(pl, out, n, c, h, w, 4, 8, 8, win, 7, 2, bad[i]);
            RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, 8, 8, bad[i]);
        }
        const int eb[] = {2, 4, 8};
        for (int i = 0; i < 3; ++i) {
            CR(pl, out, n, c, h, w, eb[i], 8, 8, win, 7, 1, SL_PLANES_AREA);
            CR(pl, out, n, c, h, w, eb[i], 8, 8, win, 7, 2, SL_PLANES_AREA);
            RS(pl, out, n, c, h, w, eb[i], 8, 8, win, 7, 1, 8, 8, SL_PLANES_AREA);
        }
    }
    /* exactly one bound zero; a negative bound; a resizing call under a shrink */
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, 8, 0, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, 0, 8, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, -1, -1, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, -8, 8, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, 8, -2147483647 - 1, SL_PLANES_AREA);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 1, 0, -1, SL_PLANES_AREA);
    RS(pl, out, n, c, h, w, 2, 8, 8, win, 7, 2, 8, 8, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 4, 8, 8, SL_PLANES_AREA);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 7, 0, 8, 8, SL_PLANES_NEAREST);
    /* what sl_normalize_view_shrink refuses: the shrink, the mask, a window that does not fit (transposed too) */
    {
        const int bad[] = {0, 3, 8, -2, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) CR(pl, out, n, c, h, w, 1, 8, 8, win, 7, bad[i], SL_PLANES_NEAREST);
    }
    CR(pl, out, n, c, h, w, 2, 8, 8, win, 8, 1, SL_PLANES_NEAREST);
    CR(pl, out, n, c, h, w, 2, 8, 8, win, -1, 1, SL_PLANES_NEAREST);
    CR(pl, out, n, c, h, w, 4, 65, 8, win, 6, 1, SL_PLANES_NEAREST);
    CR(pl, out, n, c, h, w, 4, 8, 49, win, 6, 1, SL_PLANES_NEAREST);
    CR(pl, out, n, c, h, w, 4, 64, 48, win, 7, 1, SL_PLANES_NEAREST);        /* fits as it is, not transposed */
    CR(pl, out, n, c, h, w, 1, 33, 8, win, 6, 2, SL_PLANES_AREA);
    CR(pl, out, n, c, h, w, 1, 16, 13, win, 6, 4, SL_PLANES_AREA);
    CR(pl, out, n, c, h, w, 8, 32, 24, win, 7, 2, SL_PLANES_NEAREST);        /* 64 x 48 fits, 48 x 64 does not */
    /* what sl_normalize_view_resize refuses: the mask, the bounds against the tile, their area, the scaled coordinates */
    RS(pl, out, n, c, h, w, 1, 8, 8, win, 8, 1, 8, 8, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 8, win, -1, 1, 8, 8, SL_PLANES_AREA);
    RS(pl, out, n, c, h, w, 2, 8, 8, win, 7, 1, 65, 48, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 2, 8, 8, win, 7, 1, 64, 49, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 2, 8, 8, win, 6, 1, 48, 64, SL_PLANES_NEAREST);  /* the bound is in the TILE's orientation */
    RS(pl, out, n, c, 4096, 4096, 1, 224, 224, win, 7, 1, 2049, 2048, SL_PLANES_AREA);
    RS(pl, out, n, c, 4096, 4096, 4, 224, 224, win, 0, 1, 4096, 4096, SL_PLANES_NEAREST);
    RS(pl, out, n, c, 16384, 16384, 8, 1024, 1024, win, 0, 1, 16384, 16384, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 2147483647, 8, win, 0, 1, 64, 48, SL_PLANES_NEAREST);
    RS(pl, out, n, c, h, w, 1, 8, 33554432, win, 6, 1, 64, 48, SL_PLANES_NEAREST);      /* 2^25 x 64 */
    /* n c planes, and n c patches, beyond a 32-bit grid */
    CR(pl, out, 65536, 32768, h, w, 1, 8, 8, win, 7, 1, SL_PLANES_NEAREST);             /* n c = 2^31 */
    CR(pl, out, 2147483647, 2147483647, h, w, 1, 8, 8, win, 7, 1, SL_PLANES_NEAREST);
    CR(pl, out, 2147483647, 1, 128, 128, 1, 65, 65, win, 7, 1, SL_PLANES_NEAREST);      /* 4 patches each */
    CR(pl, out, 32768, 32768, 128, 128, 2, 65, 65, win, 7, 1, SL_PLANES_NEAREST);       /* 2^30 planes x 4 patches */
    CR(pl, out, 1073741824, 1, 128, 128, 1, 17, 17, win, 7, 4, SL_PLANES_AREA);         /* 2^30 planes x 4 patches of 16 */
    RS(pl, out, 2147483647, 1, 128, 128, 4, 65, 65, win, 7, 1, 128, 128, SL_PLANES_NEAREST);
    RS(pl, out, 32768, 32768, 128, 128, 1, 65, 65, win, 7, 1, 128, 128, SL_PLANES_AREA);
    return report();
}

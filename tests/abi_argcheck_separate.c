/* Argument checks of the stain-separation entry points of the C ABI (include/stainlib_hip.h: sl_default_separate_out,
 * sl_stain_separate) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything is launched or
 * dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-separate` (tests/test_separate_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlSeparateOut is a host pointer: the undersized copy below sits at the very end of its heap block, so a library that read a
 * caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    uint8_t* o1 = (uint8_t*)0x200000;  uint8_t* o2 = (uint8_t*)0x210000;  uint8_t* o3 = (uint8_t*)0x220000;
    void* cc = (void*)0x230000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;
    const int n = 4, h = 64, w = 48;
    SlSeparateOut f;
    sl_default_separate_out(0);         /* must not crash */
    memset(&f, 0xff, sizeof f);
    sl_default_separate_out(&f);
    EXPECT(f.struct_size, sizeof(SlSeparateOut));
    EXPECT(f.conc_dtype == SL_DTYPE_F32 && !f.norm && !f.stain[0] && !f.stain[1] && !f.conc, 1);
    EXPECT(sl_version(), SL_VERSION);
    f.norm = o1; f.stain[0] = o2; f.stain[1] = o3; f.conc = cc;      /* a complete request: every refusal below is its own */

#define SEP(rgb_, n_, h_, w_, ms_, cs_, mt_, ct_, outs_) \
        EXPECT(sl_stain_separate(rgb_, n_, h_, w_, ms_, cs_, mt_, ct_, 0.01, outs_, 0), SL_ERR_BADARG)

    /* required pointers */
    SEP(0, n, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, h, w, 0, d2, d6, d2, &f);
    SEP(rgb, n, h, w, d6, 0, d6, d2, &f);
    SEP(rgb, n, h, w, d6, d2, d6, d2, 0);
    SEP(rgb, n, h, w, d6, d2, 0, 0, 0);
    /* a one-sided target */
    SEP(rgb, n, h, w, d6, d2, 0, d2, &f);
    SEP(rgb, n, h, w, d6, d2, d6, 0, &f);
    /* shapes */
    SEP(rgb, 0, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, -1, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, 0, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, h, -5, d6, d2, d6, d2, &f);
    SEP(rgb, n, 65536, 65536, d6, d2, d6, d2, &f);      /* more than 2^30 pixels */
    SEP(rgb, n, 32768, 32769, d6, d2, 0, 0, &f);        /* just over, no target */
    /* struct_size */
    {
        SlSeparateOut g = f;
        g.struct_size = 0;                         SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.struct_size = sizeof(SlSeparateOut) - 8; SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.struct_size = sizeof(SlSeparateOut) + 8; SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        void* blk = undersized(&f);                /* (the header fields and one pointer) */
        SEP(rgb, n, h, w, d6, d2, d6, d2, (const SlSeparateOut*)blk);
        SEP(rgb, n, h, w, d6, d2, 0, 0, (const SlSeparateOut*)blk);
        free(blk);
    }
    /* conc_dtype: checked with and without planes */
    {
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            SlSeparateOut g = f;
            g.conc_dtype = bad[i];  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
            g.conc = 0;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        }
    }
    /* no output */
    {
        SlSeparateOut g;
        sl_default_separate_out(&g);
        SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        SEP(rgb, n, h, w, d6, d2, 0, 0, &g);
        g.conc_dtype = SL_DTYPE_BF16;  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
    }
    /* two outputs at one address; an output at rgb */
    {
        SlSeparateOut g;
        g = f; g.stain[0] = g.norm;          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = g.norm;          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = g.stain[0];      SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.norm;              SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.stain[0];          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.stain[1];          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.norm = rgb;                 SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[0] = rgb;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = rgb;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = rgb;                 SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        sl_default_separate_out(&g); g.stain[1] = rgb;   SEP(rgb, n, h, w, d6, d2, 0, 0, &g);
    }
    /* conc aligned to its element size */
    {
        SlSeparateOut g = f;
        g.conc = (char*)cc + 1;  g.conc_dtype = SL_DTYPE_F16;   SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc_dtype = SL_DTYPE_BF16;                            SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc_dtype = SL_DTYPE_F32;                             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc = (char*)cc + 2;                                  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
    }
    return report();
}

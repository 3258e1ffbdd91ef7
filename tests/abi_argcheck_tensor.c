/* Argument checks of the tensor-output entry points of the C ABI (include/stainlib_hip.h: sl_default_tensor_format, sl_to_tensor,
 * sl_normalize_apply_tensor) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything is launched
 * or dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-tensor`
 * (tests/test_tensor_format_host.py).  The data pointers are DEVICE pointers the host side never reads through: the non-null ones
 * below are deliberately wild.  SlTensorFormat is a host pointer: the undersized copy below sits at the very end of its heap block, so
 * a library that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;  void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;     double* d2 = (double*)0x300100;
    const int n = 4, h = 64, w = 48;
    SlTensorFormat f;
    sl_default_tensor_format(0);        /* must not crash */
    memset(&f, 0xff, sizeof f);
    sl_default_tensor_format(&f);
    EXPECT(f.struct_size, sizeof(SlTensorFormat));
    EXPECT(f.dtype == SL_DTYPE_F32 && f.layout == SL_LAYOUT_NCHW && f.reserved == 0, 1);
    for (int c = 0; c < 3; ++c) EXPECT(f.mean[c] == 0.0 && f.std[c] == 1.0, 1);
    EXPECT(sl_version(), SL_VERSION);

#define BOTH(rgb_, out_, n_, h_, w_, fmt_) do { \
        EXPECT(sl_to_tensor(rgb_, out_, n_, h_, w_, fmt_, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_apply_tensor(rgb_, out_, n_, h_, w_, d6, d2, d6, d2, 0.01, fmt_, 0), SL_ERR_BADARG); } while (0)

    /* pointers and shapes */
    BOTH(0, out, n, h, w, &f);
    BOTH(rgb, 0, n, h, w, &f);
    BOTH(rgb, out, 0, h, w, &f);
    BOTH(rgb, out, -1, h, w, &f);
    BOTH(rgb, out, n, 0, w, &f);
    BOTH(rgb, out, n, h, -5, &f);
    BOTH(rgb, out, n, 65536, 65536, &f);             /* more than 2^30 pixels */
    BOTH(rgb, out, n, 32768, 32769, &f);             /* just over */
    BOTH(rgb, out, n, h, w, 0);                      /* no format */
    /* the statistics of the apply pass */
    EXPECT(sl_normalize_apply_tensor(rgb, out, n, h, w, 0, d2, d6, d2, 0.01, &f, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_apply_tensor(rgb, out, n, h, w, d6, 0, d6, d2, 0.01, &f, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_apply_tensor(rgb, out, n, h, w, d6, d2, 0, d2, 0.01, &f, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_apply_tensor(rgb, out, n, h, w, d6, d2, d6, 0, 0.01, &f, 0), SL_ERR_BADARG);
    /* struct_size */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                          BOTH(rgb, out, n, h, w, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8; BOTH(rgb, out, n, h, w, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8; BOTH(rgb, out, n, h, w, &g);
        void* blk = undersized(&f);
        BOTH(rgb, out, n, h, w, (const SlTensorFormat*)blk);
        free(blk);
    }
    /* dtype and layout */
    {
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            SlTensorFormat g = f;
            g.dtype = bad[i];  BOTH(rgb, out, n, h, w, &g);
            g = f;
            g.layout = bad[i] == 3 ? 2 : bad[i];  BOTH(rgb, out, n, h, w, &g);
        }
    }
    /* mean: finite; std: finite and > 0 */
    for (int c = 0; c < 3; ++c) {
        const double bad_mean[] = {NAN, INFINITY, -INFINITY};
        const double bad_std[] = {0.0, -0.0, -1.0, NAN, INFINITY, -INFINITY};
        for (unsigned i = 0; i < sizeof(bad_mean) / sizeof(bad_mean[0]); ++i) {
            SlTensorFormat g = f;
            g.mean[c] = bad_mean[i];  BOTH(rgb, out, n, h, w, &g);
        }
        for (unsigned i = 0; i < sizeof(bad_std) / sizeof(bad_std[0]); ++i) {
            SlTensorFormat g = f;
            g.std[c] = bad_std[i];  BOTH(rgb, out, n, h, w, &g);
        }
    }
    return report();
}

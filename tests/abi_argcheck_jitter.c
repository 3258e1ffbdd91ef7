/* Argument checks of the stain-jitter entry point of the C ABI (include/stainlib_hip.h: sl_normalize_jitter) on the HOST side, no GPU
 * needed: every refused call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under
 * AddressSanitizer by `make -C stainlib_amd/csrc asan-jitter` (tests/test_jitter_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlParams and SlTensorFormat are host pointers: the undersized copies below sit at the very end of their heap blocks, so a library
 * that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    const int n = 4, h = 64, w = 48;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

#define JIT(rgb_, out_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) \
        EXPECT(sl_normalize_jitter(rgb_, out_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, 0), SL_ERR_BADARG)
/* every refusal with and without a format, with and without a target's SlParams */
#define BOTH(rgb_, out_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_) do { \
        JIT(rgb_, out_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, 0, 0, 0); JIT(rgb_, out_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, 1, &p, &f); } while (0)

    /* required pointers */
    BOTH(0, out, n, h, w, d6, d2, d6, d2, ab);
    BOTH(rgb, 0, n, h, w, d6, d2, d6, d2, ab);
    BOTH(rgb, out, n, h, w, 0, d2, d6, d2, ab);
    BOTH(rgb, out, n, h, w, d6, 0, d6, d2, ab);
    BOTH(rgb, out, n, h, w, d6, d2, d6, d2, 0);
    BOTH(rgb, out, n, h, w, d6, d2, 0, 0, 0);           /* no target */
    /* a one-sided target */
    BOTH(rgb, out, n, h, w, d6, d2, 0, d2, ab);
    BOTH(rgb, out, n, h, w, d6, d2, d6, 0, ab);
    /* shapes */
    BOTH(rgb, out, 0, h, w, d6, d2, d6, d2, ab);
    BOTH(rgb, out, -1, h, w, d6, d2, d6, d2, ab);
    BOTH(rgb, out, n, 0, w, d6, d2, d6, d2, ab);
    BOTH(rgb, out, n, h, -5, d6, d2, d6, d2, ab);
    BOTH(rgb, out, n, 65536, 65536, d6, d2, d6, d2, ab);    /* more than 2^30 pixels */
    BOTH(rgb, out, n, 32768, 32769, d6, d2, 0, 0, ab);      /* just over, no target */
    /* SlParams.struct_size */
    {
        SlParams q = p;
        q.struct_size = 0;                         JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, &q, 0);
        q.struct_size = sizeof(SlParams) - 8;      JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, &q, &f);
        q.struct_size = sizeof(SlParams) + 8;      JIT(rgb, out, n, h, w, d6, d2, 0, 0, ab, 1, &q, 0);
        void* blk = undersized(&p);
        JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0);
        JIT(rgb, out, n, h, w, d6, d2, 0, 0, ab, 1, (const SlParams*)blk, &f);
        free(blk);
    }
    /* SlTensorFormat: struct_size, dtype, layout, std, non-finite values (the checks of sl_to_tensor) */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                               JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, &p, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      JIT(rgb, out, n, h, w, d6, d2, 0, 0, ab, 1, 0, &g);
        void* blk = undersized(&f);
        JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, (const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.layout = bad[i];                    JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = -1.0;                      JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = NAN;                       JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = INFINITY;                  JIT(rgb, out, n, h, w, d6, d2, 0, 0, ab, 1, &p, &g);
            g = f; g.mean[c] = NAN;                      JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.mean[c] = -INFINITY;                JIT(rgb, out, n, h, w, d6, d2, d6, d2, ab, 0, 0, &g);
        }
    }
    return report();
}

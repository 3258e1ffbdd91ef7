/* The frame every tests/abi_argcheck*.c driver stands in: the counters, EXPECT, the report line the tests look for, and the undersized
 * struct of a caller built against an older header. */
#ifndef ABI_ARGCHECK_H
#define ABI_ARGCHECK_H
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/stainlib_hip.h"

static int checks = 0, failed = 0;
#define EXPECT(expr, want) do { long long got_ = (long long)(expr); ++checks; \
    if (got_ != (long long)(want)) { ++failed; printf("FAIL line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got_, (long long)(want)); } } while (0)

/* A caller built against a smaller struct: the first 16 bytes of the ABI struct at s, struct_size (the first member of each) = 16, at the
 * very end of a heap block -- a library that read the struct before checking struct_size would be caught reading past it.  free() it. */
static inline void* undersized(const void* s) {
    char* blk = (char*)malloc(16);
    memcpy(blk, s, 16);
    *(uint32_t*)blk = 16;
    return blk;
}

static inline int report(void) {
    printf("%s: %d checks, %d failed\n", failed ? "FAILED" : "OK", checks, failed);
    return failed ? 1 : 0;
}
#endif

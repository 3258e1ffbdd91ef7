// view_kernels.hpp -- random crop, flip and quarter turn fused into the output sweep of the apply pass (an extension: a training loader
// crops / flips / rotates every tile differently BEHIND our call, one or two more trips over the widest data type).
//
//   k_view   per tile a window of the image that sl_normalize_jitter / sl_normalize_apply would write (or of the source bytes
//            themselves), flipped and turned by the tile's dihedral code, as the uint8 image or the model-ready tensor
//
// Definition (include/stainlib_hip.h, sl_normalize_view): the result is "the same bits, elsewhere" -- the tensor value is defined on
// the truncated byte and a dihedral transform is a permutation -- so the pixel arithmetic below is k_apply's / k_apply_jitter's
// statement for statement (apply_consts, apply_px, apply_conc, the two casts, JitterK, is_tissue_f, cvt_chunk) on the same constants.
// The kernel's body is view_body: k_view instantiates it as it stands, k_hed_view (hed_view_kernels.hpp) with the HED stage.  Its
// geometry, read side, LDS stage and write side are callable pieces (ViewTile, ViewPatch, view_read, view_stage, view_write), which
// k_lab_view (lab_view_kernels.hpp) puts around the Lab map.
// What the resizing and the affine views (view_resize_kernels.hpp, view_affine_kernels.hpp) take from here besides those pieces:
//   view_route      the route arithmetic per source pixel -- raw / failed fit / k_apply's sweep / k_apply_jitter's sweep with its
//                   constants and barriers --, ONE copy for view_resize_body and k_view_affine.  view_body holds the same text written
//                   out (its twin: folding it costs the tissue-only k_hed_view an occupancy step).
//   view_store_px4  the store tail of a write side from four packed pixels on: affine_write's.  view_write_s and resize_write hold
//                   the same text written out (twins: both measured slower on the shared function).
// Two copies of the route arithmetic where there were three; which kernel changed by how much and the timings: DESIGN 4.19.1.
//
// Shape: ONE workgroup = one tile and one patch of kViewB x kViewB OUTPUT pixels.  The dihedral code (block-uniform, read once, a
// run-time value) decides which kViewB x kViewB block of the source window that is; the two sides meet in LDS:
//   read side   walks the SOURCE block along source rows: 16 lanes per row, a 12-byte chunk (4 pixels) each, 16 rows per pass, 4 passes,
//               all four loads issued before the first arithmetic.  A row segment starts at byte 3 (y w + x0), any residue mod 4: the
//               loads are dwordx3 at byte addresses (full speed on gfx950, as in the unaligned k_apply), never predicated -- rows and
//               chunks past the block re-read its last row / chunk, a chunk that would pass the tile's end starts early and is shifted
//               into place (load12: load_chunk's rule at an arbitrary byte) -- and the LDS write is masked instead.
//   LDS         one packed dword r | g << 8 | b << 16 per pixel (the three TRUNCATED bytes), in SOURCE orientation, row pitch
//               kViewPitch = 65 dwords.
//   write side  walks OUTPUT rows: 16 lanes per row, 4 adjacent output pixels each -> one 12-byte chunk -> cvt_chunk -> 12 / 16 / 24 /
//               48 contiguous bytes per lane and plane, vector stores at element alignment; the ragged last lane of a row stores
//               element by element.  The dihedral code is only the affine map (a0, ai, aj) from output to LDS index.
// LDS banking (ds_write_b32 / ds_read_b32: bank (a / 4) % 32 within each 32-lane half; a half = 2 rows x 16 lanes): with the odd
// pitch the bank of pixel (r, x) is (r + x) % 32.  A lane's instruction s touches x = 4 c + s (c = 0..15), so on the row-wise side
// lanes c and c + 8 of a row share a bank and the next row is shifted by one: 2-way.  On the column-wise side (odd codes) the lane
// stride is 4 pitches = 4 banks, the same picture: 2-way, where an even pitch would make it 16-way.  Chosen: pitch 65 with this plain
// 4-pixels-per-lane assignment; the remaining 2-way conflict on 8 of the ~20 LDS instructions of a chunk could be rotated away
// (instruction s takes pixel (s + rot) & 3, rot per lane) at 16 selects per chunk -- not done, the pass is not LDS bound.
//
// Box shrink (sl_normalize_view_shrink): with s = 2 or 4 an output pixel is the rounded mean of an s x s box of `full`.  The
// 64 x 64 SOURCE block, the read side and the LDS stage stay as they are; one patch becomes 64 / s OUTPUT pixels square, ViewPatch maps it
// to its s nu x s nv source block with the affine map at strides s ai, s aj, and the write side gathers s s LDS dwords per output pixel
// (view_box: the packed dword as two words of 16-bit lanes, sums <= 4080, no carry), rounds, repacks and goes on through cvt_chunk and the
// stores as before.  Lanes: 4 adjacent output pixels each, 16 / s per output row: 256 busy lanes at s = 2, 64 (the first wave) at s = 4.
// Where s lives: a block-uniform RUN-TIME kernel argument for the geometry (a few scalar multiplies), and a compile-time S for the write
// side alone, picked by one scalar branch (view_write).  A template parameter of the kernels would triple the 32 + 32 + 16 instantiations
// of k_view, k_hed_view and k_lab_view -- each a copy of the per-source-pixel arithmetic, which does not depend on s -- and their build
// time; this way a code object grows by two write sides.  S = 1 is the write side as it was, statement for statement.
// Banks of the strided reads (pitch 65: bank (r + x) % 32; a 32-lane half of an instruction reads one (a, b) of the box of one p):
//   s = 2  8 lanes per output row, 4 rows per half: the lane strides are 8 and 2 banks (row-wise: 8 columns, 2 rows; column-wise the
//          other way round, 8 pitches = 8 banks) -> lanes c and c + 4 of a row share a bank, the rows fall between: 2-way, as at s = 1.
//   s = 4  4 lanes per output row, 8 rows per half: strides 16 and 4 banks -> bank 4 ((r + 4 c) % 8): 32 lanes on 8 banks, 4-way.  One
//          wave issues 64 such reads per patch, behind 4096 source pixels of arithmetic: left as it is.
#pragma once
#include "jitter_kernels.hpp"        // JitterK, the {gamma, od32} table; tensor_kernels.hpp and apply_pass.hpp through it
#include "view_geometry.hpp"         // kViewB, kViewPitch, Dihedral, ViewTile, ViewPatch

namespace sl {

constexpr int kViewRaw = 0, kViewApply = 1, kViewJitTissue = 2, kViewJitAll = 3;     // which pass `full` is

typedef uint32_t sl_u32x2u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t sl_u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// The 12 bytes at byte `base` (< nbytes) of a tile, bytes past the tile's end as zeros: load_chunk's unaligned rule (start early enough
// to stay inside, shift into place) at an arbitrary byte.  No predicated load; a tile of fewer than 12 bytes goes byte by byte.
__device__ __forceinline__ Chunk load12(const uint8_t* tile, size_t nbytes, size_t base) {
    if (nbytes < 12) return load_chunk<false>(tile + base, nbytes - base, 0);      // (uniform; its byte path clamps every address)
    const size_t lim = nbytes - 12;
    const size_t at = base < lim ? base : lim;
    const sl_u32x3u u = *(SL_GLOBAL const sl_u32x3u*)(as_global(tile) + at);
    const uint32_t d = (uint32_t)(base - at);                // 0 except at the tile's end (1..11 bytes too early)
    const uint32_t step = d >> 2, sh = 8u * (d & 3u);
    const uint32_t a0 = step == 0 ? u.x : (step == 1 ? u.y : u.z);
    const uint32_t a1 = step == 0 ? u.y : (step == 1 ? u.z : 0u);
    const uint32_t a2 = step == 0 ? u.z : 0u;
    Chunk r;
    r.w0 = (uint32_t)((((unsigned long long)a1 << 32) | a0) >> sh);
    r.w1 = (uint32_t)((((unsigned long long)a2 << 32) | a1) >> sh);
    r.w2 = a2 >> sh;
    return r;
}

// 4 output pixels (v[3 px + c], cvt_chunk's order) of one output row at pixel `pix` of the tile's oh x ow output; nvalid of them
// exist (1..4).  NCHW: `base` = the tile's plane 0, planes PO elements apart; NHWC: `base` = the tile's first element.
template <int DT, int LAYOUT>
__device__ __forceinline__ void store_view4(typename Elem<DT>::type* base, size_t PO, size_t pix, int nvalid, const float* v) {
    typedef Elem<DT> E;
    typedef typename E::type T;
    if (nvalid == 4) {
        if (LAYOUT == kLayNCHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pl[4] = {v[c], v[3 + c], v[6 + c], v[9 + c]};
                T* p = base + (size_t)c * PO + pix;
                if (DT == kDtF32) {
                    sl_u32x4u o; o.x = E::word(pl); o.y = E::word(pl + 1); o.z = E::word(pl + 2); o.w = E::word(pl + 3);
                    *(SL_GLOBAL sl_u32x4u*)as_global((uint8_t*)p) = o;
                } else {
                    sl_u32x2u o; o.x = E::word(pl); o.y = E::word(pl + 2);
                    *(SL_GLOBAL sl_u32x2u*)as_global((uint8_t*)p) = o;
                }
            }
        } else {
            uint8_t* p = (uint8_t*)(base + 3 * pix);
            if (DT == kDtF32) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    sl_u32x4u o; o.x = E::word(v + 4 * k); o.y = E::word(v + 4 * k + 1); o.z = E::word(v + 4 * k + 2); o.w = E::word(v + 4 * k + 3);
                    *(SL_GLOBAL sl_u32x4u*)as_global(p + 16 * k) = o;
                }
            } else {
                sl_u32x4u o; o.x = E::word(v); o.y = E::word(v + 2); o.z = E::word(v + 4); o.w = E::word(v + 6);
                *(SL_GLOBAL sl_u32x4u*)as_global(p) = o;
                sl_u32x2u o2; o2.x = E::word(v + 8); o2.y = E::word(v + 10);
                *(SL_GLOBAL sl_u32x2u*)as_global(p + 16) = o2;
            }
        }
    } else {
#pragma unroll
        for (int px = 0; px < 3; ++px) {
            if (px < nvalid) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    as_global(base)[LAYOUT == kLayNCHW ? (size_t)c * PO + pix + px : 3 * (pix + px) + c] = E::one(v[3 * px + c]);
            }
        }
    }
}

// The store tail of a write side: four packed pixels r | g << 8 | b << 16 of one output row at pixel `pix` of tile `tile`, nvalid of them
// existing (1 .. 4), as the uint8 image (one dwordx3, the ragged last lane byte by byte) or through cvt_chunk / store_view4.  PO: the
// pixels of a tile's output, F: tensor_consts of the call's format.  affine_write ends in it; view_write_s below and resize_write keep
// their own copies of these lines -- its twins: a change to one is a change to the others (DESIGN 4.19.1 for why they are not folded).
template <int DT, int LAYOUT>
__device__ __forceinline__ void view_store_px4(const uint32_t (&px)[4], void* out, int tile, size_t PO, size_t pix, int nvalid,
                                               const TensorK& F) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;
    typedef typename Elem<SDT>::type T;
    Chunk o;
    o.w0 = px[0] | (px[1] << 24);
    o.w1 = (px[1] >> 8) | (px[2] << 16);
    o.w2 = (px[2] >> 16) | (px[3] << 8);
    if (TENSOR) {
        float v[12];
        cvt_chunk(o, F, v);
        T* const base = (T*)out + (size_t)tile * 3 * PO;
        store_view4<SDT, LAYOUT>(base, PO, pix, nvalid, v);
    } else {
        uint8_t* const p = (uint8_t*)out + ((size_t)tile * PO + pix) * 3;
        if (nvalid == 4) {
            sl_u32x3u u; u.x = o.w0; u.y = o.w1; u.z = o.w2;
            *(SL_GLOBAL sl_u32x3u*)as_global(p) = u;
        } else {
            for (int i = 0; i < 3 * nvalid; ++i) as_global(p)[i] = (uint8_t)chunk_byte(o, i);
        }
    }
}

// ---- the pieces of a view pass: geometry, read side, LDS stage, write side.  view_body below is their sequence for one patch per
// ---- workgroup; k_lab_view (lab_view_kernels.hpp) loops them over a run of patches behind one table fill ------------------------------
// (the geometry -- Dihedral, ViewTile, ViewPatch -- is in view_geometry.hpp)

// ---- read side: the four chunks of this lane (lr = tid >> 4, lc = tid & 15), requested before any arithmetic
__device__ __forceinline__ void view_read(const ViewPatch& g, const uint8_t* src, size_t nbytes, int w, int lr, int lc, Chunk (&in)[4]) {
    const int cc = min(lc, (g.nv - 1) >> 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = min(16 * q + lr, g.nu - 1);
        in[q] = load12(src, nbytes, 3 * ((size_t)(g.ys + r) * w + g.xs) + 12 * cc);
    }
}

// the four packed pixels r | g << 8 | b << 16 of a chunk
__device__ __forceinline__ void view_unpack(const Chunk& o, uint32_t (&px)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) px[p] = chunk_pixel(o, p) & 0xffffffu;
}

// ---- LDS stage: compute(chunk, px[4]) on each of the four chunks, the pixels of the source block into s_px (masked)
template <class F>
__device__ __forceinline__ void view_stage(const ViewPatch& g, uint32_t* s_px, int lr, int lc, const Chunk (&in)[4], F&& compute) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 16 * q + lr;
        uint32_t px[4];
        compute(in[q], px);
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (r < g.nu && 4 * lc + p < g.nv) s_px[r * kViewPitch + 4 * lc + p] = px[p];
    }
}

// The rounded mean of the S x S box of packed pixels whose first pixel is s_px[at] (S = 2, 4): the packed dword as two words of 16-bit
// lanes -- r and b in px & 0xff00ff, g in (px >> 8) & 0xff --, whose sums (at most 16 x 255 = 4080, + S S / 2) cannot carry into the next
// lane; (sum + S S / 2) >> 2 log2 S is round half up, and the bits the shift moves across a lane's edge are masked off.
template <int S>
__device__ __forceinline__ uint32_t view_box(const uint32_t* s_px, int at) {
    static_assert(S == 2 || S == 4, "a 2 x 2 or 4 x 4 box");
    constexpr int SH = S == 2 ? 2 : 4;                       // log2 of the pixels of a box
    constexpr uint32_t HALF = (uint32_t)(S * S / 2);
    uint32_t rb = HALF | (HALF << 16), gg = HALF;
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
        for (int b = 0; b < S; ++b) {
            const uint32_t px = s_px[at + a * kViewPitch + b];
            rb += px & 0x00ff00ffu;
            gg += (px >> 8) & 0xffu;
        }
    return ((rb >> SH) & 0x00ff00ffu) | ((gg >> SH) << 8);
}

// A stage on the WRITE side, between the four packed pixels of an output row and their packing into a Chunk: the post stage of
// sl_normalize_post_view (post_kernels.hpp: PostStage), which acts on OUTPUT pixels and needs their index in the tile's output.  The
// default is empty -- kOn = false: the hook's statement is discarded and every other kernel's code is what it was (tools/isa_diff.py).
// apply(px, g, il, jl, ow): the lane holds the outputs (il, jl .. jl + 3) of patch g, some of which may not exist.
struct ViewNoPost {
    static constexpr bool kOn = false;
    __device__ __forceinline__ void apply(uint32_t (&)[4], const ViewPatch&, int, int, int) const {}
};

// ---- write side: output rows, 4 adjacent pixels per lane (behind a barrier after the stage).  S: the shrink, a compile-time value HERE
// ---- only (view_write below picks it by the block-uniform run-time one); S = 1 is the write side as it was, statement for statement.
// Lanes: 16 / S per output row (the patch is 64 / S pixels wide), so 16 S rows per pass -- 4 passes at S = 1, ONE at S = 2 (32 rows, every
// lane busy) and at S = 4 (16 rows: the first wave only; accepted, the pass is bound by the arithmetic in front of the stage).
// From `Chunk o` on this is view_store_px4's text written out, its TWIN (the S = 1 float16 view was 1 - 2 % slower on it).
template <int DT, int LAYOUT, int S, class Post = ViewNoPost>
__device__ __forceinline__ void view_write_s(const ViewPatch& g, const uint32_t* s_px, void* out, int tile, int oh, int ow, TensorK fmt,
                                             int lr16, int lc16, const Post& post = Post()) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;
    constexpr int LPR = 16 / S, NPASS = S == 1 ? 4 : 1;      // lanes per output row, passes
    typedef typename Elem<SDT>::type T;
    const int i0 = g.i0, j0 = g.j0, bh = g.bh, bw = g.bw, a0 = g.a0, ai = g.ai, aj = g.aj;
    const TensorK F = tensor_consts(fmt);
    const size_t PO = (size_t)oh * ow;
    const int lr = S == 1 ? lr16 : (16 * lr16 + lc16) / LPR, lc = S == 1 ? lc16 : lc16 % LPR;
    const int jl = 4 * lc;
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
        const int il = 16 * q + lr;
        const int row = a0 + min(il, bh - 1) * ai;
        uint32_t px[4];
        if constexpr (S == 1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) px[p] = s_px[row + min(jl + p, bw - 1) * aj];
        } else {
            if (il >= bh || jl >= bw) continue;              // (whole waves at S = 4; nothing below has a barrier)
#pragma unroll
            for (int p = 0; p < 4; ++p) px[p] = view_box<S>(s_px, row + min(jl + p, bw - 1) * aj);
        }
        if constexpr (Post::kOn) post.apply(px, g, il, jl, ow);
        Chunk o;
        o.w0 = px[0] | (px[1] << 24);
        o.w1 = (px[1] >> 8) | (px[2] << 16);
        o.w2 = (px[2] >> 16) | (px[3] << 8);
        const int nvalid = min(4, bw - jl);
        if (il < bh && nvalid > 0) {
            const size_t pix = (size_t)(i0 + il) * ow + (j0 + jl);
            if (TENSOR) {
                float v[12];
                cvt_chunk(o, F, v);
                T* const base = (T*)out + (size_t)tile * 3 * PO;
                store_view4<SDT, LAYOUT>(base, PO, pix, nvalid, v);
            } else {
                uint8_t* const p = (uint8_t*)out + ((size_t)tile * PO + pix) * 3;
                if (nvalid == 4) {
                    sl_u32x3u u; u.x = o.w0; u.y = o.w1; u.z = o.w2;
                    *(SL_GLOBAL sl_u32x3u*)as_global(p) = u;
                } else {
                    for (int i = 0; i < 3 * nvalid; ++i) as_global(p)[i] = (uint8_t)chunk_byte(o, i);
                }
            }
        }
    }
}

// the write side of a patch under the run-time shrink s (block-uniform: one scalar branch)
template <int DT, int LAYOUT, class Post = ViewNoPost>
__device__ __forceinline__ void view_write(const ViewPatch& g, const uint32_t* s_px, void* out, int tile, int oh, int ow, TensorK fmt,
                                           int lr, int lc, int s, const Post& post = Post()) {
    if (s == 1) view_write_s<DT, LAYOUT, 1>(g, s_px, out, tile, oh, ow, fmt, lr, lc, post);
    else if (s == 2) view_write_s<DT, LAYOUT, 2>(g, s_px, out, tile, oh, ow, fmt, lr, lc, post);
    else view_write_s<DT, LAYOUT, 4>(g, s_px, out, tile, oh, ow, fmt, lr, lc, post);
}

// A further stage between the truncation to bytes and the LDS write, on the four packed pixels `stage` holds.  HED = 0: none -- the
// primary template is empty and k_view's code is what it was without it (tools/isa_diff.py); HED = 1: the HED augmentation of
// sl_normalize_hed_view (hed_view_kernels.hpp specialises it; its arguments arrive in HedViewArgs).
struct HedViewArgs {
    const double *sigma, *bias;      // n x 3 each (device)
    const int32_t* applied;          // n (device): the tile takes the stage or not
    double H[9], R[9];               // hed_from_rgb, rgb_from_hed (row-major)
};
template <int HED>
struct HedStage {
    __device__ __forceinline__ void init(int, int, const HedViewArgs*) {}
    __device__ __forceinline__ void apply(uint32_t (&)[4]) const {}
};
// HED = 2: the HSB map of sl_normalize_hsb_view (hsb_kernels.hpp specialises the stage; its arguments arrive in a struct of their own).
// StageArgs<HED>: what view_body and view_resize_body hand to the stage's init.
struct HsbViewArgs;
template <int HED> struct StageArgs { typedef HedViewArgs type; };
template <> struct StageArgs<2> { typedef HsbViewArgs type; };

// ---- the route arithmetic per source pixel of the staged view kernels: between the read side (the loads are in flight, the table fill is
// ---- issued) and the barrier in front of the write side.  stage(compute) runs compute(chunk, px[4]) on the lane's four chunks and puts the
// ---- pixels into LDS (the caller's view_stage, with its HedStage behind compute); s_tab: the {gamma, od32} table (MODE != kViewRaw).
// view_resize_body and k_view_affine call it; view_body below holds the same text written out -- its twin: a change to one is a change
// to the other (DESIGN 4.19.1 for why view_body is not folded).  HED == 1: the raw stage waits for the HED stage's table.
template <int MODE, int HED, class Stage>
__device__ __forceinline__ void view_route(const float2* s_tab, Stage&& stage, int npatch, int P, const uint8_t* rgb,
                                           const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                           const double* alpha_beta, double lam, float ylimf) {
    auto unpack = [](const Chunk& o, uint32_t (&px)[4]) { view_unpack(o, px); };
    auto raw = [&](const Chunk& c, uint32_t (&px)[4]) { unpack(c, px); };

    if (MODE == kViewRaw) {
        if (HED == 1) __syncthreads();                              // the HED stage's table
        stage(raw);
    } else {
        const ApplyTile<1> A(blockIdx.x, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
        const ApplyK& K = A.K;
        JitterK J;
        if (MODE != kViewApply) {                                   // k_apply_jitter's constants
            const double sc = 1.0 / A.unit;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                J.al[i] = in_vgpr(uni((float)alpha_beta[4 * (size_t)A.tile + 2 * i]));
                J.be[i] = in_vgpr(uni((float)(alpha_beta[4 * (size_t)A.tile + 2 * i + 1] / (A.mct[i] / A.mcs[i]) * sc)));
            }
            J.ylimf = in_vgpr(ylimf);
        }
        __syncthreads();                                            // the table
        if (SL_FIT_FAILED(A)) {                                     // the view of the source bytes
            stage(raw);
        } else if (MODE == kViewApply) {                            // k_apply: K.fast picks the lasso form and the cast
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                stage([&](const Chunk& c, uint32_t (&px)[4]) {
                    float t[12];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float x = s_tab[chunk_byte(c, 3 * p + 0)].y, y = s_tab[chunk_byte(c, 3 * p + 1)].y,
                                    z = s_tab[chunk_byte(c, 3 * p + 2)].y;
                        float v[3];
                        apply_px<FAST>(K, x, y, z, v);
                        t[3 * p] = v[0]; t[3 * p + 1] = v[1]; t[3 * p + 2] = v[2];
                    }
                    unpack(FAST ? pack_trunc_fast(t) : pack_trunc_general(t), px);
                });
            };
            if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
        } else {                                                    // k_apply_jitter: g12 picks the lasso form, the cast saturates
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                stage([&](const Chunk& c, uint32_t (&px)[4]) {
                    float t[12];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float2 er = s_tab[chunk_byte(c, 3 * p + 0)];      // x = gamma, y = od32
                        const float2 eg = s_tab[chunk_byte(c, 3 * p + 1)];
                        const float2 eb = s_tab[chunk_byte(c, 3 * p + 2)];
                        float c1, c2;
                        apply_conc<FAST>(K, er.y, eg.y, eb.y, c1, c2);
                        if (MODE == kViewJitAll) {
                            c1 = fmaf(c1, J.al[0], J.be[0]);
                            c2 = fmaf(c2, J.al[1], J.be[1]);
                        } else {
                            const bool tissue = is_tissue_f(er.x, eg.x, eb.x, J.ylimf);
                            c1 = tissue ? fmaf(c1, J.al[0], J.be[0]) : c1;
                            c2 = tissue ? fmaf(c2, J.al[1], J.be[1]) : c2;
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            t[3 * p + ch] = 255.0f * __builtin_amdgcn_exp2f(fmaf(c1, K.q[0][ch], c2 * K.q[1][ch]));
                    }
                    unpack(pack_trunc_fast(t), px);
                });
            };
            if (K.L.g12 >= 0.0f) sweep(std::true_type{}); else sweep(std::false_type{});
        }
    }
}

// DT: kDtU8 or a tensor type; LAYOUT: tensor only; MODE: kView*; HED: the stage above.  npx: patches per output row, npatch: per tile.
// From `unpack` to the last barrier this is view_route's text written out, its TWIN: a change to one is a change to the other.  Calling
// view_route here costs the tissue-only k_hed_view an occupancy step (79 -> 81 VGPRs, 6 -> 5).
// Post: the write-side stage (ViewNoPost: none); a PostStage has filled its table before the call, behind the barrier below.
template <int DT, int LAYOUT, int MODE, int HED, class Post = ViewNoPost>
__device__ __forceinline__ void view_body(const uint8_t* rgb, void* out, int h, int w, int oh, int ow,
                                          int npx, int npatch, const int32_t* windows, int d_mask, int shrink,
                                          const double* M_src, const double* maxC_src,
                                          const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
                                          double lam, float ylimf, TensorK fmt, const typename StageArgs<HED>::type* hv,
                                          const Post& post = Post()) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;
    HedStage<HED> hed;
    hed.init(tid, tile, hv);

    // the view of this tile (block-uniform), the source block of this patch and the four chunks of this lane
    const int s = __builtin_amdgcn_readfirstlane(shrink);
    const ViewTile vt(windows, tile, d_mask, h, w, oh, ow, s);
    const ViewPatch g(vt, patch, npx, oh, ow, s);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) {
            compute(c, px);
            hed.apply(px);
        });
    };
    auto unpack = [](const Chunk& o, uint32_t (&px)[4]) { view_unpack(o, px); };
    auto raw = [&](const Chunk& c, uint32_t (&px)[4]) { unpack(c, px); };

    if (MODE == kViewRaw) {
        if (HED == 1) __syncthreads();                              // the HED stage's table
        stage(raw);
    } else {
        const ApplyTile<1> A(blockIdx.x, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
        const ApplyK& K = A.K;
        JitterK J;
        if (MODE != kViewApply) {                                   // k_apply_jitter's constants
            const double sc = 1.0 / A.unit;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                J.al[i] = in_vgpr(uni((float)alpha_beta[4 * (size_t)A.tile + 2 * i]));
                J.be[i] = in_vgpr(uni((float)(alpha_beta[4 * (size_t)A.tile + 2 * i + 1] / (A.mct[i] / A.mcs[i]) * sc)));
            }
            J.ylimf = in_vgpr(ylimf);
        }
        __syncthreads();                                            // the table
        if (SL_FIT_FAILED(A)) {                                     // the view of the source bytes
            stage(raw);
        } else if (MODE == kViewApply) {                            // k_apply: K.fast picks the lasso form and the cast
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                stage([&](const Chunk& c, uint32_t (&px)[4]) {
                    float t[12];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float x = s_tab[chunk_byte(c, 3 * p + 0)].y, y = s_tab[chunk_byte(c, 3 * p + 1)].y,
                                    z = s_tab[chunk_byte(c, 3 * p + 2)].y;
                        float v[3];
                        apply_px<FAST>(K, x, y, z, v);
                        t[3 * p] = v[0]; t[3 * p + 1] = v[1]; t[3 * p + 2] = v[2];
                    }
                    unpack(FAST ? pack_trunc_fast(t) : pack_trunc_general(t), px);
                });
            };
            if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
        } else {                                                    // k_apply_jitter: g12 picks the lasso form, the cast saturates
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                stage([&](const Chunk& c, uint32_t (&px)[4]) {
                    float t[12];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float2 er = s_tab[chunk_byte(c, 3 * p + 0)];      // x = gamma, y = od32
                        const float2 eg = s_tab[chunk_byte(c, 3 * p + 1)];
                        const float2 eb = s_tab[chunk_byte(c, 3 * p + 2)];
                        float c1, c2;
                        apply_conc<FAST>(K, er.y, eg.y, eb.y, c1, c2);
                        if (MODE == kViewJitAll) {
                            c1 = fmaf(c1, J.al[0], J.be[0]);
                            c2 = fmaf(c2, J.al[1], J.be[1]);
                        } else {
                            const bool tissue = is_tissue_f(er.x, eg.x, eb.x, J.ylimf);
                            c1 = tissue ? fmaf(c1, J.al[0], J.be[0]) : c1;
                            c2 = tissue ? fmaf(c2, J.al[1], J.be[1]) : c2;
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            t[3 * p + ch] = 255.0f * __builtin_amdgcn_exp2f(fmaf(c1, K.q[0][ch], c2 * K.q[1][ch]));
                    }
                    unpack(pack_trunc_fast(t), px);
                });
            };
            if (K.L.g12 >= 0.0f) sweep(std::true_type{}); else sweep(std::false_type{});
        }
    }
    __syncthreads();

    view_write<DT, LAYOUT>(g, s_px, out, tile, oh, ow, fmt, lr, lc, s, post);
}

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                     int npx, int npatch, const int32_t* __restrict__ windows, int d_mask, int shrink,
                                                     const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                     const double* M_tgt, const double* maxC_tgt, const double* __restrict__ alpha_beta,
                                                     double lam, float ylimf, TensorK fmt) {
    view_body<DT, LAYOUT, MODE, 0>(rgb, out, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam,
                                   ylimf, fmt, nullptr);
}

}  // namespace sl

// Device helpers shared by the fused-MLP translation units (mlp_fp32.hip, mlp_16.hip,
// mlp_dw.hip, mlp_pack.hip): operand types and conversions, the positional encoding,
// B-operand image access, the scalar-loaded vector / pair images, and the dX kernels'
// active-tile selection.
#pragma once

#include <type_traits>
#include <utility>

#include "common.hpp"
#include "mfma.hpp"
#include "mlp_plan.hpp"

namespace nr {

// 16-bit MFMA operands (bf16 or fp16; both stored as 16-bit patterns in bf16x8
// registers, the MFMA and the conversions pick the format) or fp32.
template <int PREC>
constexpr bool k16 = PREC != NR_PREC_FP32;

template <int PREC>
struct InBlk {
    bf16x8 s[2];
};
template <>
struct InBlk<NR_PREC_FP32> {
    f32x16 v;
};

template <int PREC>
constexpr int kFPB = k16<PREC> ? 2 : 4;  // 1-KB fragments per 32x32 block

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// D += A.B on 16-bit operand images of either format
template <int PREC>
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (PREC == NR_PREC_FP16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
                                                      0, 0, 0);
    else
        return mfma_bf16(a, b, c);
}

// Two fp32 -> one word of two bf16 (RNE), low half = lo: one v_cvt_pk_bf16_f32
// (element-wise casts compile to one convert per element plus a v_perm per pair;
// not inline asm: the hazard recognizer does not see an asm def that an MFMA reads).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
template <int PREC>
__device__ __forceinline__ unsigned cvt_pk16(float lo, float hi) {
    if constexpr (PREC == NR_PREC_FP16)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, f16x2));
    else
        return cvt_pk_bf16(lo, hi);
}
// 16-bit pattern of x (round to nearest even)
template <int PREC>
__device__ __forceinline__ float from16_lo(unsigned w) {
    if constexpr (PREC == NR_PREC_FP16)
        return static_cast<float>(__builtin_bit_cast(f16x2, w)[0]);
    else
        return __uint_as_float(w << 16);
}

// registers 8 hf .. 8 hf + 7 of an accumulator as a 16-bit operand
template <int PREC = NR_PREC_BF16>
__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int hf) {
    u32x4 w;
#pragma unroll
    for (int m = 0; m < 4; ++m) w[m] = cvt_pk16<PREC>(a[8 * hf + 2 * m], a[8 * hf + 2 * m + 1]);
    return __builtin_bit_cast(bf16x8, w);
}

template <int PREC>
__device__ __forceinline__ void to_in(const f32x16& a, InBlk<PREC>& o) {
    if constexpr (k16<PREC>) {
        o.s[0] = pack8<PREC>(a, 0);
        o.s[1] = pack8<PREC>(a, 1);
    } else {
        o.v = a;
    }
}

__device__ __forceinline__ void zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

#ifndef NR_SIN
#define NR_SIN sinf
#define NR_COS cosf
#endif
// lane * 16 recomputed in place (2 VALU): lane-derived offsets are otherwise kept
// live across the whole kernel, and under register pressure spilled and
// reloaded with a vmcnt(0) that also drains the in-flight weight stream.
__device__ __forceinline__ uint32_t lane16() {
    uint32_t v;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshlrev_b32 %0, 4, %0" : "=v"(v));
    return v;
}

// Positional-encoding feature f of a 3-vector (model.py:72-80): [x | sin 2^0 x | cos 2^0 x | ...].
__device__ __forceinline__ float pe_feat(float x0, float x1, float x2, int f, int L) {
    if (f < 3) return f == 0 ? x0 : (f == 1 ? x1 : x2);
    const int fp = f - 3;
    const int k = fp / 6;
    if (k >= L) return 0.f;  // padding column
    const int rem = fp - 6 * k;
    const int c = rem % 3;
    const float xv = c == 0 ? x0 : (c == 1 ? x1 : x2);
    const float v = exp2f(static_cast<float>(k)) * xv;
    return rem < 3 ? NR_SIN(v) : NR_COS(v);
}

// d gamma_f / d x_c contracted with g (torch: (g * cos(fx)) * f, (g * -sin(fx)) * f).
__device__ __forceinline__ void pe_feat_bwd(float x0, float x1, float x2, int f, int L, float g, float& g0,
                                            float& g1, float& g2) {
    int c;
    float d;
    if (f < 3) {
        c = f;
        d = g;
    } else {
        const int fp = f - 3;
        const int k = fp / 6;
        if (k >= L) return;
        const int rem = fp - 6 * k;
        c = rem % 3;
        const float xv = c == 0 ? x0 : (c == 1 ? x1 : x2);
        const float fr = exp2f(static_cast<float>(k));
        const float v = fr * xv;
        d = rem < 3 ? (g * cosf(v)) * fr : (g * -sinf(v)) * fr;
    }
    // selects, not branches: the branches became a run-time-indexed scratch array
    g0 += c == 0 ? d : 0.f;
    g1 += c == 1 ? d : 0.f;
    g2 += c == 2 ? d : 0.f;
}

// bf16 positional encoding.  sin/cos by the hardware v_sin_f32 (argument in
// revolutions) after an exact two-term reduction: x/(2 pi) = hi + lo with
// hi = x*C1 rounded and lo = fma(x, C1, -hi) + x*C2, so 2^k x/(2 pi) mod 1 =
// fract(2^k hi) + 2^k lo (2^k hi exact).  Absolute error ~1e-6, far below the
// bf16 rounding (2^-9 relative) the encoding goes through; the fp32 path keeps
// sinf/cosf.  cos(v) = sin(v + 1/4 revolution).
struct PeRev {
    float x[3], hi[3], lo[3];
};

__device__ __forceinline__ PeRev pe_rev(float x0, float x1, float x2) {
    constexpr float C1 = 0.15915494f, C2 = 6.4206382e-09f;  // fp32(1/2pi), 1/2pi - C1
    PeRev p;
    const float xs[3] = {x0, x1, x2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p.x[c] = xs[c];
        p.hi[c] = xs[c] * C1;
        p.lo[c] = fmaf(xs[c], C1, -p.hi[c]) + xs[c] * C2;
    }
    return p;
}

// feature f (compile-time after unrolling) for lane half 0 and f1 for half 1
__device__ __forceinline__ float pe_fast(const PeRev& p, int f0, int f1, bool h1, int L) {
    auto kind = [](int f) { return f < 3 ? 0 : 1; };
    auto trig = [&](int f, float& hi, float& lo) {  // 2^k (hi, lo) + phase of feature f
        const int fp = f - 3, k = fp / 6, rem = fp - 6 * k, c = rem % 3;
        const float sc = static_cast<float>(1 << (k < 24 ? k : 0));
        hi = p.hi[c] * sc;
        lo = fmaf(p.lo[c], sc, rem < 3 ? 0.f : 0.25f);
        return k < L;
    };
    if (kind(f0) == 1 && kind(f1) == 1) {
        float h0, l0, hh, lh;
        const bool v0 = trig(f0, h0, l0), v1 = trig(f1, hh, lh);
        const float hi = h1 ? hh : h0, lo = h1 ? lh : l0;
        const float v = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(hi) + lo);
        return (h1 ? v1 : v0) ? v : 0.f;
    }
    auto one = [&](int f) -> float {
        if (f < 3) return p.x[f];
        float hi, lo;
        const bool ok = trig(f, hi, lo);
        return ok ? __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(hi) + lo) : 0.f;
    };
    const float a0 = one(f0), a1 = one(f1);
    return h1 ? a1 : a0;
}

// Backward of pe_fast: d gamma_f / d x_c contracted with g, for feature f0 (lane
// half 0) / f1 (half 1).  d sin(theta + phi)/d theta = sin(theta + phi + 1/4 rev), so
// the derivative is the same hardware sine a quarter revolution on (sin -> cos,
// cos -> -sin), times 2^k.  16-bit paths only (the fp32 path keeps sinf/cosf).
__device__ __forceinline__ void pe_fast_bwd(const PeRev& p, int f0, int f1, bool h1, int L, float g, float& g0,
                                            float& g1, float& g2) {
    auto chan = [](int f) { return f < 3 ? f : ((f - 3) - 6 * ((f - 3) / 6)) % 3; };
    // selects: a run-time index into p.hi / p.lo put them in scratch
    auto sel = [](const float (&v)[3], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); };
    auto live = [&](int f) { return f < 3 || (f - 3) / 6 < L; };
    auto dgamma = [&](int f) -> float {  // d gamma_f / d x_c (f >= 3, live)
        const int fp = f - 3, k = fp / 6, rem = fp - 6 * k, c = rem % 3;
        const float sc = static_cast<float>(1 << (k < 24 ? k : 0));
        const float hi = sel(p.hi, c) * sc, lo = fmaf(sel(p.lo, c), sc, rem < 3 ? 0.25f : 0.5f);
        return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(hi) + lo) * sc;
    };
    float d;
    if (f0 >= 3 && f1 >= 3) {
        const int fp0 = f0 - 3, k0 = fp0 / 6, r0 = fp0 - 6 * k0;
        const int fp1 = f1 - 3, k1 = fp1 / 6, r1 = fp1 - 6 * k1;
        const float s0 = static_cast<float>(1 << (k0 < 24 ? k0 : 0)), s1 = static_cast<float>(1 << (k1 < 24 ? k1 : 0));
        const float hi = h1 ? sel(p.hi, r1 % 3) * s1 : sel(p.hi, r0 % 3) * s0;
        const float lo = h1 ? fmaf(sel(p.lo, r1 % 3), s1, r1 < 3 ? 0.25f : 0.5f) : fmaf(sel(p.lo, r0 % 3), s0, r0 < 3 ? 0.25f : 0.5f);
        d = g * (__builtin_amdgcn_sinf(__builtin_amdgcn_fractf(hi) + lo) * (h1 ? s1 : s0));
    } else {
        const float a0 = f0 < 3 ? 1.f : (live(f0) ? dgamma(f0) : 0.f);
        const float a1 = f1 < 3 ? 1.f : (live(f1) ? dgamma(f1) : 0.f);
        d = g * (h1 ? a1 : a0);
    }
    if (!(h1 ? live(f1) : live(f0))) return;
    const int c = h1 ? chan(f1) : chan(f0);
    g0 += c == 0 ? d : 0.f;
    g1 += c == 1 ? d : 0.f;
    g2 += c == 2 ? d : 0.f;
}

// ---- bf16 epilogue: bias by MFMA, ReLU and mask bits on packed bf16 pairs ----
// Bias of row block nb as an MFMA A fragment against an all-ones B operand:
// lanes 0..31 hold bias[32 nb + lane] split exactly into bf16 hi + mid + lo,
// lanes 32..63 zeros, so D += bias broadcast over the 32 samples of the tile.
template <int PREC>
__device__ __forceinline__ bf16x8 bias_frag(float b) {
    const unsigned w0 = cvt_pk16<PREC>(b, 0.f);            // hi
    const float r1 = b - from16_lo<PREC>(w0);
    const unsigned w1 = cvt_pk16<PREC>(r1, 0.f);           // mid
    const float r2 = r1 - from16_lo<PREC>(w1);
    const unsigned w2 = cvt_pk16<PREC>(r2, 0.f);           // lo
    return __builtin_bit_cast(bf16x8, u32x4{w0 | (w1 << 16), w2, 0u, 0u});
}

template <int PREC>
__device__ __forceinline__ bf16x8 ones16() {
    const unsigned one = PREC == NR_PREC_FP16 ? 0x3C003C00u : 0x3F803F80u;
    return __builtin_bit_cast(bf16x8, u32x4{one, one, one, one});
}

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// Word w (0..7) of a bf16 block holds accumulator registers 2w (low half) and
// 2w+1 (high half).  bf16 ReLU = max as int16 against 0 (negative bf16 has the
// sign bit set).  Mask bits of a layer, 4 words per lane: block nb, word w sets
// bit j = 8 (nb & 1) + w (register 2w > 0) and bit 16 + j (register 2w+1 > 0)
// of word nb >> 1.
__device__ __forceinline__ unsigned relu_pk(unsigned w) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, w), s16x2{0, 0}));
}
// (asm: after the ReLU the compiler knows w >= 0 and rewrites the min into
// per-half compares and selects, six instructions instead of one)
__device__ __forceinline__ unsigned nz_pk(unsigned w) {
    unsigned r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(w), "s"(0x10001u));
    return r;
}

// One accumulator block (bias included) -> its 16-bit B operand: pack, ReLU on the
// packed pairs, mask bits.
template <int PREC, bool RELU, bool MASK>
__device__ __forceinline__ void epi16_blk(const f32x16& a, bf16x8 (&out)[2], unsigned* mw, int nb) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        u32x4 wd = __builtin_bit_cast(u32x4, pack8<PREC>(a, hf));
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if constexpr (RELU) wd[m] = relu_pk(wd[m]);
            if constexpr (MASK) mw[nb >> 1] |= nz_pk(wd[m]) << (8 * (nb & 1) + 4 * hf + m);
        }
        out[hf] = __builtin_bit_cast(bf16x8, wd);
    }
}

// Backward: zero the packed dz pairs whose forward activation was not positive.
__device__ __forceinline__ void mask_pk(bf16x8 (&v)[2], unsigned word, int nb) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        u32x4 wd = __builtin_bit_cast(u32x4, v[hf]);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const unsigned t = (word >> (8 * (nb & 1) + 4 * hf + m)) & 0x10001u;
            wd[m] &= t * 0xFFFFu;
        }
        v[hf] = __builtin_bit_cast(bf16x8, wd);
    }
}

// dz block -> B operand with the ReLU mask of its forward activation applied
// (bf16: packed-pair mask words of epi16_blk; fp32: bit (nb&1)*16 + r of word nb>>1).
template <int PREC>
__device__ __forceinline__ void to_in_masked(f32x16 a, const u32x4& mw, int nb, InBlk<PREC>& o) {
    if constexpr (k16<PREC>) {
        to_in<PREC>(a, o);
        mask_pk(o.s, mw[nb >> 1], nb);
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned bit = (mw[nb >> 1] >> ((nb & 1) * 16 + r)) & 1u;
            a[r] = bit ? a[r] : 0.f;
        }
        o.v = a;
    }
}

// One 32-feature block of a tile as a B-operand image: FPB fragments of 1 KB.
template <int PREC>
__device__ __forceinline__ void store_img(char* __restrict__ region, int64_t tile, int nblk, int blk,
                                          const InBlk<PREC>& v) {
    // wave-uniform base (tile is per wave) + the lane's 16 B: saddr + voffset stores
    char* base = region + ((tile * nblk + blk) * kFPB<PREC>) * static_cast<int64_t>(kFragBytes) + lane16();
    if constexpr (k16<PREC>) {
        // streaming (non-temporal) stores: the 4 GB of images must not evict the
        // L2-resident weight stream every workgroup re-reads
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v.s[0]), reinterpret_cast<u32x4*>(base));
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v.s[1]), reinterpret_cast<u32x4*>(base + kFragBytes));
    } else {
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
            *reinterpret_cast<f32x4*>(base + tq * kFragBytes) =
                f32x4{v.v[4 * tq], v.v[4 * tq + 1], v.v[4 * tq + 2], v.v[4 * tq + 3]};
    }
}

template <int PREC>
__device__ __forceinline__ void load_img(const char* __restrict__ region, int64_t tile, int nblk, int blk,
                                         InBlk<PREC>& v) {
    const char* base = region + ((tile * nblk + blk) * kFPB<PREC>) * static_cast<int64_t>(kFragBytes) + lane16();
    if constexpr (k16<PREC>) {
        v.s[0] = *reinterpret_cast<const bf16x8*>(base);
        v.s[1] = *reinterpret_cast<const bf16x8*>(base + kFragBytes);
    } else {
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(base + tq * kFragBytes);
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[4 * tq + e] = q[e];
        }
    }
}

// Vector images (mlp_plan.hpp; biases, w_sigma, W_rgb: 16 fp32 per (block, lane half)) are
// read with SCALAR loads through the constant address space and selected per
// lane half, so they cost no vector registers; the opaque pointer copy keeps the
// loads from being hoisted out of the layer loops as invariants.
typedef const __attribute__((address_space(4))) float cfloat;

struct VImg {
    cfloat* p;
    bool hi;
    // registers 4g..4g+3 of block nb, for this lane's half
    __device__ __forceinline__ f32x4 g4(int nb, int g) const {
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = p[(2 * nb) * 16 + 4 * g + e], up = p[(2 * nb + 1) * 16 + 4 * g + e];
            r[e] = hi ? up : lo;
        }
        return r;
    }
};

__device__ __forceinline__ VImg vimg(const char* packed, int64_t off, int lane) {
    const char* q = packed + off;
    asm volatile("" : "+s"(q));
    return VImg{(cfloat*)(q), (lane >> 5) != 0};
}
#define NR_VEC(img, nb, g) ((img).g4((nb), (g)))

// Pair images (w_sigma, the rows of W_rgb): element nb*16 + r holds the weights of
// accumulator register r of block nb for lane half 0 and for lane half 1, read with
// one 64-bit scalar load; a packed FMA evaluates both halves and each lane keeps
// its own (no per-lane selects of scalar weights: VOP3 reads one SGPR at most).
typedef const __attribute__((address_space(4))) f32x2 cf32x2;
struct PImg {
    cf32x2* p;
    __device__ __forceinline__ f32x2 at(int nb, int r) const { return p[nb * 16 + r]; }
};
__device__ __forceinline__ PImg pimg(const char* packed, int64_t off) {
    const char* q = packed + off;
    asm volatile("" : "+s"(q));
    return PImg{(cf32x2*)(q)};
}
__device__ __forceinline__ f32x2 bcast2(float x) { return f32x2{x, x}; }
// ReLU as an integer max (negative floats, -0 included, are negative as int32):
// one v_max_i32, where the float compare-select also canonicalises its input
__device__ __forceinline__ float relu_f(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

// ---- the ends the dX chains share (mlp_bwd_kernel, mlp_bwd_rbm_kernel, mlp_dinput_kernel) ----
// Heads backward of sample m (torch: g * (1 - y) * y for the sigmoid, g * (y > 0) for the
// ReLU), times the loss scale.  Where !valid, dr and dzs keep the caller's values (zeros).
__device__ __forceinline__ void head_grads(const float* rgb, const float* sigma, const float* g_rgb,
                                           const float* g_sigma, float gscale, int64_t m, bool valid, float (&dr)[3],
                                           float& dzs) {
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = rgb[3 * m + c];
            dr[c] = ((g_rgb[3 * m + c] * (1.0f - y)) * y) * gscale;
        }
        dzs = (sigma[m] > 0.f ? g_sigma[m] : 0.f) * gscale;
    }
}

// dz of the heads as one 32-feature block: feature 0 sigma, 1..3 rgb (lane half h)
template <int PREC>
__device__ __forceinline__ InBlk<PREC> heads_blk(int h, float dzs, const float (&dr)[3]) {
    f32x16 hb;
    zero(hb);
    if (h == 0) {
        hb[0] = dzs;
        hb[1] = dr[0];
        hb[2] = dr[1];
        hb[3] = dr[2];
    }
    InBlk<PREC> hv;
    to_in<PREC>(hb, hv);
    return hv;
}

// Tail of an input gradient: the two lane halves' sums added, and sample m's three
// components stored, the loss scale divided out (store: a valid sample's lane half 0)
__device__ __forceinline__ void store_input_grad(float* g, int64_t m, bool store, float inv_gscale, float g0,
                                                 float g1, float g2) {
    g0 += __shfl_xor(g0, 32);
    g1 += __shfl_xor(g1, 32);
    g2 += __shfl_xor(g2, 32);
    if (store) {
        g[3 * m] = g0 * inv_gscale;
        g[3 * m + 1] = g1 * inv_gscale;
        g[3 * m + 2] = g2 * inv_gscale;
    }
}

// Active tiles of a segment from its flags (tile_flags_kernel), one wave: lane l holds
// flag word l (tiles 4l .. 4l+3 of the segment, one byte each, 0 or 1), its count and the
// wave's inclusive scan of the counts.
struct SegFlags {
    uint32_t word;
    int count, incl, total;
};
__device__ __forceinline__ uint32_t seg_flag_word(const uint8_t* __restrict__ flags, int64_t sg) {
    static_assert(kSegTiles == 4 * 64, "one flag word per lane");
    return reinterpret_cast<const uint32_t*>(flags + sg * kSegTiles)[threadIdx.x & 63];
}
__device__ __forceinline__ SegFlags seg_scan(uint32_t word) {
    const int lane = threadIdx.x & 63;
    SegFlags f;
    f.word = word;
    f.count = __popc(f.word);
    f.incl = f.count;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(f.incl, d);
        if (lane >= d) f.incl += o;
    }
    f.total = __builtin_amdgcn_readfirstlane(__shfl(f.incl, 63));
    return f;
}

// The tile of the segment's k-th active tile (k < f.total; wave-uniform result).
__device__ __forceinline__ int64_t seg_entry(const SegFlags& f, int64_t sg, int k) {
    const uint64_t over = __ballot(f.incl > k);
    const int L = __builtin_ctzll(over);  // the lane whose word holds entry k
    const uint32_t w = __builtin_amdgcn_readfirstlane(__shfl(f.word, L));
    int r = k - __builtin_amdgcn_readfirstlane(__shfl(f.incl - f.count, L));
    int b = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool set = (w >> (8 * q)) & 1u;
        if (set && r == 0) b = q;
        r -= set ? 1 : 0;
        if (r < 0) r = 1 << 20;  // found: no later byte matches
    }
    return sg * kSegTiles + 4 * L + b;
}

// The dW kernel's work list: every active tile once, in increasing order, and their
// total.  Each segment's tiles are placed by wave 0 of the dX workgroup that leads the
// segment (part 0), after its own tiles, from `before` (the active tiles of the segments
// before it, select_tile): each lane writes the active tiles of its flag word.
__device__ __forceinline__ void place_segment(const SegFlags& f, uint32_t before, int64_t nseg, int64_t sg,
                                              uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    uint32_t slot = before + static_cast<uint32_t>(f.incl - f.count);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if ((f.word >> (8 * q)) & 1u) list[slot++] = static_cast<uint32_t>(sg * kSegTiles + 4 * lane + q);
    if (sg == nseg - 1 && lane == 0) *count = before + static_cast<uint32_t>(f.total);
}

// A dX wave's tile.  Every workgroup reads the 64-tile block counts of the whole launch
// (tile_flags_kernel; one uint4 per segment, from L2) and its segment's flags, in one
// round of loads:
//  * every tile active (the dense case: bare-init training, cfg->dense_backward):
//    workgroup b runs tiles W b .. W b + W - 1, the layout's own order (no lists; dW
//    takes its identity path on count == tiles);
//  * otherwise, segment-minor: workgroup b takes part j = b / nseg of segment
//    (b - j) mod nseg, i.e. the active tiles W j .. W j + W - 1 of that segment, so the
//    workgroups with active tiles are dispatched first and spread over every XCD
//    (blocks are dealt to XCDs round-robin); parts past a segment's count have nothing
//    to do.
// Measured (fine bf16 M=786432 dX, profiles/r06_tile_map_ab.txt): segment-minor in the
// dense case costs ~7 % at M=786432 and ~20 % at 262144 (locality), segment-major in
// the skipping case 1.67x at 37 % active.
constexpr int64_t kDenseCheckSegs = 1024;  // launches up to 262,144 tiles check for "all active"

struct TileSel {
    SegFlags sf;
    int64_t seg, tile;
    uint32_t before;   // skipping form: active tiles of the segments before seg
    bool dense, live, idle, leader;
};
__device__ __forceinline__ TileSel select_tile(const uint8_t* __restrict__ flags,
                                               const uint32_t* __restrict__ blk_count, int64_t nseg,
                                               int64_t tiles, int W, int wv) {
    constexpr int BPS = kSegTiles / 64;  // 64-tile blocks per segment
    const int lane = threadIdx.x & 63;
    const int64_t b = blockIdx.x;
    TileSel t;
    // skipping form: part-major over the segments (the parts with active tiles go first),
    // the segment rotated by the part, so that one segment's parts land on different
    // XCDs (b % 8) even when nseg is a multiple of 8: segments whose counts differ (a
    // trained field's rays hit or miss as a whole) then load every XCD alike
    const int part = static_cast<int>(b / nseg);
    t.seg = (b % nseg + nseg - part % nseg) % nseg;
    // every load first (one round trip): the segment's flag word and the block counts,
    // one uint4 (a segment's four blocks) per lane and 64 segments.  Past
    // kDenseCheckSegs segments (M > 8.4M samples) reading every count in every workgroup
    // would grow with M^2: such launches take the skipping form, which is right for any
    // flags, and only the leaders read the counts before their segment
    static_assert(BPS == 4, "a segment's block counts are one uint4");
    const bool check = nseg <= kDenseCheckSegs;  // launch-uniform
    const int64_t lim = check ? nseg : (part == 0 && wv == 0 ? t.seg : 0);
    const uint32_t word = seg_flag_word(flags, t.seg);
    const uint4* __restrict__ bc4 = reinterpret_cast<const uint4*>(blk_count);
    uint32_t all = 0, before = 0;
    for (int64_t s0 = 0; s0 < lim; s0 += 4 * 64) {
        uint4 c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t sg = s0 + i * 64 + lane;
            c[i] = sg < lim ? bc4[sg] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t n = ((c[i].x + c[i].y) + c[i].z) + c[i].w;
            all += n;
            before += (s0 + i * 64 + lane) < t.seg ? n : 0u;
        }
    }
    t.sf = seg_scan(word);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        all += __shfl_xor(all, d);
        before += __shfl_xor(before, d);
    }
    t.before = __builtin_amdgcn_readfirstlane(before);
    t.dense = check && static_cast<int64_t>(__builtin_amdgcn_readfirstlane(all)) == tiles;
    if (t.dense) {
        const int64_t first = b * W;
        t.tile = first + wv;
        t.live = t.tile < tiles;
        t.idle = first >= tiles;
        t.leader = b == 0 && wv == 0;
    } else {
        const int k = part * W + wv;
        t.idle = part * W >= t.sf.total;
        t.live = k < t.sf.total;
        t.tile = t.live ? seg_entry(t.sf, t.seg, k) : 0;
        t.leader = part == 0 && wv == 0;
    }
    return t;
}

// the leader's share of the dW list (skipping form) or the dense count
__device__ __forceinline__ void finish_tiles(const TileSel& t, int64_t nseg, int64_t tiles, uint32_t* __restrict__ list,
                                             uint32_t* __restrict__ count) {
    if (!t.leader) return;
    if (t.dense) {
        if ((threadIdx.x & 63) == 0) *count = static_cast<uint32_t>(tiles);
    } else {
        place_segment(t.sf, t.before, nseg, t.seg, list, count);
    }
}

// compile-time loop: f(integral_constant<int, j>) for j = 0..NN-1
template <int... Js, class F>
__device__ __forceinline__ void rbm_static_for(std::integer_sequence<int, Js...>, F&& f) {
    (f(std::integral_constant<int, Js>{}), ...);
}
template <int NN, class F>
__device__ __forceinline__ void rbm_static_for(F&& f) {
    rbm_static_for(std::make_integer_sequence<int, NN>{}, f);
}

}  // namespace nr

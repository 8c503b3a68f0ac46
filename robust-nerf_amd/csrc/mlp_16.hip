// 16-bit (bf16 / fp16) path of the fused NeRF MLP, ROW-BLOCK MAJOR: forward
// (mlp_fwd_rbm.inc), backward dX chain (mlp_bwd_rbm.inc) and the input gradients
// g_x / g_d as a pass over the stored dz images (mlp_dinput_kernel).
#include <algorithm>

#include "mlp_dev.hpp"
#include "mlp_launch.hpp"

namespace nr {

#include "mlp_fwd_rbm.inc"
#include "mlp_bwd_rbm.inc"

// ------------------------------------------------ input gradients ------
// dL/dx and dL/dd of the 16-bit path (the pose-optimisation gradient, BASELINE
// cfg #3) as a separate pass over the dz images the dX chain stores anyway:
//   d x_enc = sum over the x_enc-reading layers l (0 and every skip layer) of
//             W_l[:, x_enc]^T dz_l,        d d_enc = W_dir[:, d_enc]^T dz_dir,
// then the positional-encoding backward.  A dX chain that carries d x_enc through
// the whole trunk (as the fp32 mlp_bwd_kernel does for WANT_X) runs 4 waves per CU
// (2.23 ms vs 1.17 ms for the plain dX chain).
// One wave per 32-sample tile; the A fragments are the W^T images' x_enc / d_enc
// row blocks (gathered into LDS once per workgroup), the B operands the stored dz
// blocks.  fp32 accumulation, the same products as the fused variant.  HBM-bound:
// 1.28 KB of dz per sample for the default model (dz_0, dz_skip, dz_c).
struct DinArgs {
    const char* packed;
    const char* ws;
    const float* x;
    const float* d;
    float* g_x;
    float* g_d;
    int64_t M, tiles;
    const uint8_t* flags;         // active tiles (tile_flags_kernel): the others have dz == 0
    int L, Ld;
    float inv_gscale;
    int nsrc;                     // x_enc-reading layers
    int64_t a_off[kMaxTrunk];     // byte offset of the layer's W^T image
    int a_kb[kMaxTrunk];          // row blocks per chunk of that image
    int a_p0[kMaxTrunk];          // first x_enc row block within a chunk
    int64_t dz_off[kMaxTrunk];    // byte offset of the layer's dz image in ws
    int64_t dir_a_off, dz_dir_off;
    int dir_kb, dir_p0, nc;       // dir W^T chunk rows, first d_enc row, dz_dir blocks
};

constexpr int kDinNT = 512;

// The x_enc / d_enc row blocks of every source W^T image, gathered fragment by
// fragment: [source][dz block][row block][2] then [dz_c block][row block][2] (1 KB each).
__host__ __device__ inline int din_frags(int nsrc, int XB, int DB, int nc) { return 2 * (nsrc * kHB * XB + nc * DB); }

template <int PREC, int XB, int DB, bool ALDS>
__global__ __launch_bounds__(kDinNT) void mlp_dinput_kernel(DinArgs a) {
    static_assert(k16<PREC>, "16-bit images only");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63, h = lane >> 5, ml = lane & 31;
    // A operands: staged once per workgroup into LDS (72 KB for the default model), or
    // read from the L2-resident packed buffer when they do not fit
    auto frag_src = [&](int f) -> const char* {  // global address of gathered fragment f (lane 0)
        const int nx = 2 * a.nsrc * kHB * XB;
        if (f < nx) {
            const int s = f / (2 * kHB * XB), r = f % (2 * kHB * XB);
            const int ob = r / (2 * XB), q = r % (2 * XB);
            return a.packed + a.a_off[s] + static_cast<int64_t>((ob * a.a_kb[s] + a.a_p0[s]) * 2 + q) * kFragBytes;
        }
        const int r = f - nx, ob = r / (2 * DB > 0 ? 2 * DB : 1), q = r % (2 * DB > 0 ? 2 * DB : 1);
        return a.packed + a.dir_a_off + static_cast<int64_t>((ob * a.dir_kb + a.dir_p0) * 2 + q) * kFragBytes;
    };
    if constexpr (ALDS) {
        const int nf = din_frags(a.nsrc, XB, DB, a.nc);
        for (int i = threadIdx.x; i < nf * 64; i += kDinNT) {
            const int f = i >> 6, l = i & 63;
            *reinterpret_cast<u32x4*>(lds + f * kFragBytes + l * 16) =
                *reinterpret_cast<const u32x4*>(frag_src(f) + l * 16);
        }
        __syncthreads();
    }
    auto afrag = [&](int f) -> bf16x8 {
        if constexpr (ALDS)
            return *reinterpret_cast<const bf16x8*>(lds + f * kFragBytes + lane * 16);
        else
            return *reinterpret_cast<const bf16x8*>(frag_src(f) + lane * 16);
    };
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kDinNT / 64);
    for (int64_t tile = static_cast<int64_t>(blockIdx.x) * (kDinNT / 64) + (threadIdx.x >> 6); tile < a.tiles;
         tile += waves) {
        const int64_t tile_u = __builtin_amdgcn_readfirstlane(static_cast<int>(tile));
        const int64_t m = tile * 32 + ml;
        const bool valid = m < a.M;
        if (!a.flags[tile_u]) {
            // no incoming gradient in this tile: its dz were never computed, and its input
            // gradients are exactly zero
            if (valid && h == 0)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (a.g_x) a.g_x[3 * m + c] = 0.f;
                    if (a.g_d) a.g_d[3 * m + c] = 0.f;
                }
            continue;
        }
        if (a.g_x) {
            f32x16 dxe[XB];
#pragma unroll
            for (int q = 0; q < XB; ++q) zero(dxe[q]);
            for (int s = 0; s < a.nsrc; ++s) {
                InBlk<PREC> b[kHB];
#pragma unroll
                for (int ob = 0; ob < kHB; ++ob) load_img<PREC>(a.ws + a.dz_off[s], tile_u, kHB, ob, b[ob]);
#pragma unroll
                for (int ob = 0; ob < kHB; ++ob)
#pragma unroll
                    for (int q = 0; q < XB; ++q) {
                        const int f = ((s * kHB + ob) * XB + q) * 2;
                        dxe[q] = mfma16<PREC>(afrag(f), b[ob].s[0], dxe[q]);
                        dxe[q] = mfma16<PREC>(afrag(f + 1), b[ob].s[1], dxe[q]);
                    }
            }
            const PeRev pr = pe_rev(valid ? a.x[3 * m] : 0.f, valid ? a.x[3 * m + 1] : 0.f,
                                    valid ? a.x[3 * m + 2] : 0.f);
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
            for (int kb = 0; kb < XB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    pe_fast_bwd(pr, 32 * kb + acc_row(r, 0), 32 * kb + acc_row(r, 1), h != 0, a.L, dxe[kb][r], g0, g1,
                                g2);
            store_input_grad(a.g_x, m, valid && h == 0, a.inv_gscale, g0, g1, g2);
        }
        if constexpr (DB > 0) {
            if (a.g_d) {
                f32x16 dd[DB];
#pragma unroll
                for (int q = 0; q < DB; ++q) zero(dd[q]);
                const int f0 = 2 * a.nsrc * kHB * XB;
                for (int ob = 0; ob < a.nc; ++ob) {
                    InBlk<PREC> b;
                    load_img<PREC>(a.ws + a.dz_dir_off, tile_u, a.nc, ob, b);
#pragma unroll
                    for (int q = 0; q < DB; ++q) {
                        const int f = f0 + (ob * DB + q) * 2;
                        dd[q] = mfma16<PREC>(afrag(f), b.s[0], dd[q]);
                        dd[q] = mfma16<PREC>(afrag(f + 1), b.s[1], dd[q]);
                    }
                }
                const PeRev pr = pe_rev(valid ? a.d[3 * m] : 0.f, valid ? a.d[3 * m + 1] : 0.f,
                                        valid ? a.d[3 * m + 2] : 0.f);
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int kb = 0; kb < DB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        pe_fast_bwd(pr, 32 * kb + acc_row(r, 0), 32 * kb + acc_row(r, 1), h != 0, a.Ld, dd[kb][r], g0,
                                    g1, g2);
                store_input_grad(a.g_d, m, valid && h == 0, a.inv_gscale, g0, g1, g2);
            }
        }
    }
}

namespace {

template <int PREC>
int launch_dinput(const MlpPlan& p, const DinArgs& a, hipStream_t s) {
    const size_t lds = static_cast<size_t>(din_frags(a.nsrc, p.XB, p.DB, a.nc)) * kFragBytes;
    const bool alds = lds <= 160 * 1024;
    // enough workgroups for 2 per CU (the staging is amortised over ~6 tiles per wave)
    const dim3 grid(static_cast<unsigned>(std::min<int64_t>(ceil_div_ll(a.tiles, kDinNT / 64), 512))),
        block(kDinNT);
    const bool found = dispatch_model(p, [&](auto xb, auto db) {
        constexpr int XB = decltype(xb)::value, DB = decltype(db)::value;
        if (alds)
            hipLaunchKernelGGL((mlp_dinput_kernel<PREC, XB, DB, true>), grid, block, lds, s, a);
        else
            hipLaunchKernelGGL((mlp_dinput_kernel<PREC, XB, DB, false>), grid, block, 0, s, a);
    });
    if (!found) {
        set_error("nr_mlp_backward_dx: no input-gradient kernel for XB=%d DB=%d", p.XB, p.DB);
        return NR_EARG;
    }
    return check_launch("nr_mlp_backward_dx (input gradients)");
}

// TRAIN: the ReLU masks are stored; ACT: the activations too
template <int PREC, bool TRAIN, bool ACT>
int launch_fwd_rbm_t(const MlpPlan& p, const RbmArgs& a, hipStream_t s) {
    // every chunk fits a slot (checked at compile time per layer shape).  Eight waves per
    // workgroup at every size: four- and six-wave workgroups for small launches (all CUs
    // busy, or even rounds) were faster in isolation at 1,024 tiles but slower inside the
    // graph-replayed 512-ray step, where the coarse backward shares the chip
    // (profiles/r06_rbm_waves.txt; r04 found the same)
    constexpr int W = kRbmWaves;
    const dim3 grid(static_cast<unsigned>(ceil_div_ll(a.tiles, W))), block(W * 64);
    const size_t lds = rbm_lds_bytes(p.XB, W);
    const bool found = dispatch_model(p, [&](auto xb, auto db) {
        hipLaunchKernelGGL((mlp_fwd_rbm_kernel<PREC, decltype(xb)::value, decltype(db)::value, TRAIN, W, ACT>), grid,
                           block, lds, s, a);
    });
    if (!found) {
        set_error("nr_mlp_forward: no kernel instance for XB=%d DB=%d", p.XB, p.DB);
        return NR_EARG;
    }
    return check_launch("nr_mlp_forward");
}

template <int PREC, bool INPUT>
int launch_bwd_rbm_t(const MlpPlan& p, const BwdrArgs& a, hipStream_t s) {
    constexpr int W = kRbmWaves;
    // the masks of every layer in LDS where they fit (up to 10 trunk layers), else read in place
    const bool mlds = bwdr_lds_bytes(p.n_mask, W) <= 160 * 1024;
    const size_t lds = bwdr_lds_bytes(mlds ? p.n_mask : 0, W);
    // every part of every segment (mlp_bwd_rbm_kernel's workgroup mapping)
    const dim3 grid(static_cast<unsigned>(a.nseg * (kSegTiles / W))), block(W * 64);
    if (mlds)
        hipLaunchKernelGGL((mlp_bwd_rbm_kernel<PREC, W, INPUT, true>), grid, block, lds, s, a);
    else
        hipLaunchKernelGGL((mlp_bwd_rbm_kernel<PREC, W, INPUT, false>), grid, block, lds, s, a);
    return check_launch(INPUT ? "nr_mlp_backward_input" : "nr_mlp_backward_dx");
}

}  // namespace

int launch_fwd_rbm(const MlpPlan& p, const RbmArgs& a, FwdSave save, hipStream_t s) {
    return dispatch_prec16(p.prec, [&](auto prec) {
        constexpr int PREC = decltype(prec)::value;
        switch (save) {
            case FwdSave::Train: return launch_fwd_rbm_t<PREC, true, true>(p, a, s);
            case FwdSave::Masks: return launch_fwd_rbm_t<PREC, true, false>(p, a, s);
            default: return launch_fwd_rbm_t<PREC, false, false>(p, a, s);
        }
    });
}

int launch_bwd_rbm(const MlpPlan& p, const BwdrArgs& a, bool input_only, hipStream_t s) {
    return dispatch_prec16(p.prec, [&](auto prec) {
        constexpr int PREC = decltype(prec)::value;
        return input_only ? launch_bwd_rbm_t<PREC, true>(p, a, s) : launch_bwd_rbm_t<PREC, false>(p, a, s);
    });
}

// 16-bit g_x / g_d: one MFMA pass over the stored dz images of the x_enc-reading
// layers and of dz_c (mlp_dinput_kernel), after the dX chain wrote them
int input_grads16(const MlpPlan& p, const DinOffsets& o, const char* packed, const float* x, const float* d,
                  float* g_x, float* g_d, const char* ws, int64_t M, hipStream_t s) {
    const int n = p.n_layers;
    DinArgs da{};
    da.packed = packed;
    da.ws = ws;
    da.flags = reinterpret_cast<const uint8_t*>(ws + o.flags_off);
    da.x = x;
    da.d = d;
    da.g_x = g_x;
    da.g_d = g_d;
    da.M = M;
    da.tiles = o.tiles;
    da.L = p.L;
    da.Ld = p.Ld;
    da.inv_gscale = 1.0f / grad_scale(p.prec);
    // layer 0 reads x_enc alone; a skip layer's W^T chunk is [h (8) | x_enc (XB)]
    for (int l = 0; l < n; ++l) {
        if (l > 0 && !is_skip(p, l - 1)) continue;
        da.a_off[da.nsrc] = p.lin[l].pk_bwd;
        da.a_kb[da.nsrc] = p.lin[l].KB;
        da.a_p0[da.nsrc] = p.lin[l].KB - p.XB;
        da.dz_off[da.nsrc] = o.dz_off[l];
        da.nsrc++;
    }
    // dir's W^T chunk is [feat (8) | d_enc (DB)], one chunk per dz_c block
    da.dir_a_off = p.lin[n + 1].pk_bwd;
    da.dir_kb = p.lin[n + 1].KB;
    da.dir_p0 = kHB;
    da.nc = p.lin[n + 1].NB;
    da.dz_dir_off = o.dz_dir_off;
    return dispatch_prec16(p.prec, [&](auto prec) { return launch_dinput<decltype(prec)::value>(p, da, s); });
}

}  // namespace nr

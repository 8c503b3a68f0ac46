// 16-bit (bf16 / fp16) backward dX chain of the fused MLP, ROW-BLOCK MAJOR
// (included by mlp_16.hip after mlp_fwd_rbm.inc, whose stream and layer loop it reuses;
// BwdrArgs: mlp_launch.hpp).
// Reference: the autograd backward of noisy_src/model.py:145-196.
//
//   dz_heads = [g_sigma * (sigma > 0), g_rgb * (1 - rgb) * rgb]        (VALU)
//   dz_c     = (W_rgb^T dz_rgb) * [h_c > 0]                            (VALU)
//   dz_feat  = W_dir[:, feat]^T dz_c                                   (no activation)
//   dz_{n-1} = (W_feat^T dz_feat + w_sigma dz_sigma) * [h_{n-1} > 0]
//   dz_{i-1} = (W_i[:, h]^T dz_i) * [h_{i-1} > 0],   i = n-1 .. 1
//
// Each dz is stored as a B-operand image for the dW GEMM (and, for dz_0, dz_skip
// and dz_c, for the pose-optimisation input gradients, mlp_dinput_kernel).  A
// layer's W^T image (pk_bwdr) is row-block major over the hidden input rows: a
// row block's accumulator (32 input features x 32 samples) is final after its
// 2 * NB_out MFMAs and its epilogue (sigma term, ReLU mask, 16-bit pack, store)
// runs under the next row block's MFMAs.  Same products in the same k order as
// the chunk-major 16-bit chain it replaced, to which its dz images were bit-identical.
// The ReLU masks of every layer are staged into LDS once (LDS-DMA, 1 KB per
// layer and wave), so no global load waits inside the stream.  That takes 8 KB per
// masked layer beside the stream's 64 KB: up to 10 trunk layers fit the 160 KiB.  A
// deeper net runs the MLDS = false instance, which stages none and reads each layer's
// mask from global memory where the staged form reads LDS (the same words, so the same
// dz; the load is not counted in s.nvm, which only makes the next stream wait stricter).

constexpr int kBwdrSlot = 32 * 1024;  // every dX-chain chunk: 2 row blocks x 8 k blocks, or 4 x 4
__host__ __device__ constexpr int bwdr_mask_off() { return 2 * kBwdrSlot; }
__host__ __device__ constexpr int bwdr_sig_off(int n_mask, int W) { return 2 * kBwdrSlot + W * n_mask * 1024; }
__host__ __device__ constexpr int bwdr_lds_bytes(int n_mask, int W) { return bwdr_sig_off(n_mask, W) + 1024; }

// dz of a layer's hidden input: ReLU mask of the forward activation, pack, store
// (OPT: the input-only chain stores the image only when `keep`, and counts only then)
template <int PREC, bool OPT = false>
struct BwdrTrunkFin {
    InBlk<PREC> (&out)[kHB];
    u32x4 mw;
    char* dst;  // dz image
    int64_t tile;
    int& nvm;
    bool sig;            // feature layer: + w_sigma dz_sigma first
    float dzs;
    const float* wsig;   // LDS: w_sigma vector image, this lane's half
    bool keep = true;
    __device__ __forceinline__ void operator()(int rb, f32x16& a, const bf16x8&) const {
        if (sig)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wsig + rb * 32 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[4 * g + e] = fmaf(w[e], dzs, a[4 * g + e]);
            }
        to_in_masked<PREC>(a, mw, rb, out[rb]);
        if (!OPT || keep) {  // workgroup-uniform
            store_img<PREC>(dst, tile, kHB, rb, out[rb]);
            nvm += 2;
        }
    }
};

// dz_feat = d feat (feature_linear has no activation)
template <int PREC, bool STORE = true>
struct BwdrFeatFin {
    InBlk<PREC> (&out)[kHB];
    char* dst;
    int64_t tile;
    int& nvm;
    __device__ __forceinline__ void operator()(int rb, f32x16& a, const bf16x8&) const {
        to_in<PREC>(a, out[rb]);
        if constexpr (STORE) {
            store_img<PREC>(dst, tile, kHB, rb, out[rb]);
            nvm += 2;
        }
    }
};

// INPUT: the input-only chain of a frozen field (nr_mlp_backward_input).  It stores only the
// dz images mlp_dinput_kernel reads (dz_c and the trunk layers of a.keep_dz), into the
// compact workspace of FrozenSizes, builds no dW list, and reads its masks from a region
// without scratch tiles (a wave without a tile takes tile 0's: its inputs are zero and
// its stores land in its scratch tile).  s.nvm counts the stores actually issued; which
// layers store is the same for every wave of the launch.
template <int PREC, int W, bool INPUT = false, bool MLDS = true>
__global__ __launch_bounds__(W * 64, 1) void mlp_bwd_rbm_kernel(BwdrArgs a) {
    static_assert(kSegTiles % W == 0, "whole parts per segment");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, ml = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // wave -> its tile (select_tile); a workgroup without any exits.  A wave without one
    // (past a segment's count, or past the last tile) runs on zero inputs in one of the
    // kScratchTiles scratch tiles, spread so that such waves do not contend for one tile's
    // lines: it stores like the others, so every wave issues the same compile-time count
    // of vector-memory ops and each stream wait stays one s_waitcnt (the stream's
    // barriers need every wave anyway)
    const TileSel ts = select_tile(a.flags, a.blk_count, a.nseg, a.tiles, W, wv);
    if (ts.idle) {  // workgroup-uniform
        if constexpr (!INPUT) finish_tiles(ts, a.nseg, a.tiles, a.dw_list, a.count);
        return;
    }
    const int64_t tile = ts.live ? ts.tile : a.scratch_base + ((blockIdx.x * W + wv) & (kScratchTiles - 1));
    const int64_t m = tile * 32 + ml;
    const bool valid = m < a.M;
    const int n = a.n_layers;
    constexpr int NC = kHB / 2;

    // this wave's ReLU masks (n_mask KB) and w_sigma (wave 0) -> LDS; older than the
    // stream's first chunk, so its boundary wait publishes them.  The dir layer's
    // mask (needed before the stream) is also read directly.
    const int nml = MLDS ? a.n_mask : 0;  // mask KB per wave in LDS (launch_bwd_rbm_t sizes it the same way)
    char* mlds = lds + bwdr_mask_off() + wv * nml * 1024;
    const char* msrc = a.saved + a.mask_off + (INPUT && !ts.live ? 0 : tile) * a.n_mask * 1024;
    if constexpr (MLDS)
        for (int l = 0; l < a.n_mask; ++l)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(msrc + l * 1024 + lane16()),
                (__attribute__((address_space(3))) void*)(mlds + l * 1024), 16, 0, 0);
    if (wv == 0)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(a.packed + a.vhead + lane16()),
            (__attribute__((address_space(3))) void*)(lds + bwdr_sig_off(nml, W)), 16, 0, 0);
    const u32x4 mwc = *reinterpret_cast<const u32x4*>(msrc + n * 1024 + lane16());
    auto mask_of = [&](int layer) {
        if constexpr (MLDS) return *reinterpret_cast<const u32x4*>(mlds + layer * 1024 + lane16());
        else return *reinterpret_cast<const u32x4*>(msrc + layer * 1024 + lane16());
    };
    const float* wsig = reinterpret_cast<const float*>(lds + bwdr_sig_off(nml, W)) + 16 * h;

    RStream s{lds, a.packed + a.base, -1, 0, wv, kBwdrSlot, W};
    constexpr int CK_DIR = rbm_chunk_kb(NC, 0), CK_H = rbm_chunk_kb(kHB, 0);
    static_assert(CK_DIR * 1024 <= kBwdrSlot && CK_H * 1024 <= kBwdrSlot, "dX chunk");
    rbm_dma(s, CK_DIR);
    s.q = 0;

    // heads: sigmoid / relu backward
    float dr[3] = {0.f, 0.f, 0.f}, dzs = 0.f;
    head_grads(a.rgb, a.sigma, a.g_rgb, a.g_sigma, a.gscale, m, valid, dr, dzs);
    if constexpr (!INPUT) {
        store_img<PREC>(a.ws + a.ws_off[a.ws_heads], tile, 1, 0, heads_blk<PREC>(h, dzs, dr));
        s.nvm += 2;
    }
    // dz_c = (W_rgb^T dz_rgb) * [h_c > 0]
    InBlk<PREC> cin[NC];
    {
        const PImg wr0 = pimg(a.packed, a.vrgb), wr1 = pimg(a.packed, a.vrgb + NC * 128),
                   wr2 = pimg(a.packed, a.vrgb + 2 * NC * 128);
#pragma unroll
        for (int nb = 0; nb < NC; ++nb) {
            f32x16 dc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                f32x2 v = wr0.at(nb, r) * bcast2(dr[0]);
                v = __builtin_elementwise_fma(wr1.at(nb, r), bcast2(dr[1]), v);
                v = __builtin_elementwise_fma(wr2.at(nb, r), bcast2(dr[2]), v);
                dc[r] = h ? v[1] : v[0];
            }
            to_in_masked<PREC>(dc, mwc, nb, cin[nb]);
            store_img<PREC>(a.ws + a.ws_off[a.ws_dir], tile, NC, nb, cin[nb]);
            s.nvm += 2;
        }
    }

    InBlk<PREC> hA[kHB], hB[kHB];
    // dz_feat = W_dir[:, feat]^T dz_c
    {
        BwdrFeatFin<PREC, !INPUT> fin{hA, a.ws + a.ws_off[a.ws_feat], tile, s.nvm};
        auto in = [&](int kb) -> const InBlk<PREC>& { return cin[kb]; };
        rbm_layer<PREC, NC, kHB, 0, decltype(in), decltype(fin), 0>(s, CK_H, in, fin);
    }
    // dz_{n-1} = (W_feat^T dz_feat + w_sigma dz_sigma) * [h_{n-1} > 0]
    {
        BwdrTrunkFin<PREC, INPUT> fin{hB, mask_of(n - 1), a.ws + a.ws_off[WS_DZ0 + n - 1], tile, s.nvm, true, dzs,
                                      wsig, !INPUT || ((a.keep_dz >> (n - 1)) & 1u)};
        auto in = [&](int kb) -> const InBlk<PREC>& { return hA[kb]; };
        rbm_layer<PREC, kHB, kHB, 0, decltype(in), decltype(fin), 0>(s, n > 1 ? CK_H : 0, in, fin);
    }
    // dz_{i-1} = (W_i[:, h]^T dz_i) * [h_{i-1} > 0]
    auto trunk = [&](int i, InBlk<PREC>(&hin)[kHB], InBlk<PREC>(&hout)[kHB]) {
        BwdrTrunkFin<PREC, INPUT> fin{hout, mask_of(i - 1), a.ws + a.ws_off[WS_DZ0 + i - 1], tile, s.nvm, false, 0.f,
                                      wsig, !INPUT || ((a.keep_dz >> (i - 1)) & 1u)};
        auto in = [&](int kb) -> const InBlk<PREC>& { return hin[kb]; };
        rbm_layer<PREC, kHB, kHB, 0, decltype(in), decltype(fin), 0>(s, i > 1 ? CK_H : 0, in, fin);
    };
    for (int i = n - 1; i >= 1; i -= 2) {
        trunk(i, hB, hA);
        if (i == 1) break;
        trunk(i - 1, hA, hB);
    }
    if constexpr (!INPUT) finish_tiles(ts, a.nseg, a.tiles, a.dw_list, a.count);
}

// 16-bit (bf16 / fp16) forward of the fused MLP, ROW-BLOCK MAJOR (included by mlp_16.hip;
// RbmArgs: mlp_launch.hpp).
// Reference: noisy_src/model.py:145-196 (NeRF.forward), 20-80 (PositionalEncoding).
//
// Each wave owns one 32-sample tile.  A layer's packed image is row-block major:
// per 32-row block, its 2*KB k-step A fragments followed by its bias fragment
// (bias_frag: hi/mid/lo split, lanes 0..31), so one stream chunk = R whole row
// blocks (24-42 KB) of one layer, and a row block's accumulator is final after
// its 2*KB MFMAs.  Its epilogue (bias MFMA, 16-bit packing, ReLU, mask bits,
// saved-activation store, head FMAs) then runs while the NEXT row block
// multiplies, instead of all eight epilogues following the layer's last chunk.
// The layer input h_{i-1} and the output h_i being built both stay in registers
// (8 blocks = 64 VGPRs each, ping-pong over pairs of layers); LDS holds only the
// weight ring (two 42-KB slots).  Same operands, same per-row-block accumulation
// order (k ascending) and the same epilogue arithmetic as the chunk-major 16-bit
// kernel it replaced, to which its results were bit-identical.
//
// Stream protocol (two slots): at the boundary of chunk q every wave waits for its
// own LDS-DMA pieces of chunk q (a counted vmcnt: the saved-activation stores it
// issued since stay in flight), then barriers, then issues chunk q+1 into the other
// slot (last read during chunk q-1, which every wave finished before the barrier).

constexpr int kRbmSlot = 42 * 1024;
// waves (tiles) per workgroup; the kernels take it as a template argument (W), the
// launches use 8 (launch_fwd_rbm_t says why)
constexpr int kRbmWaves = 8;
// LDS: the two ring slots, each wave's x_enc image (the skip layer's leading k
// blocks), the head weights (w_sigma, W_rgb rows) as per-lane-half vector images
__host__ __device__ constexpr int rbm_xenc_off() { return 2 * kRbmSlot; }
__host__ __device__ constexpr int rbm_head_off(int XB, int W) { return 2 * kRbmSlot + W * XB * 2 * kFragBytes; }
__host__ __device__ constexpr int rbm_lds_bytes(int XB, int W) { return rbm_head_off(XB, W) + 3 * 1024; }

struct RStream {
    char* lds;
    const char* src;  // next chunk to load
    int q;            // chunk being consumed
    int nvm;          // vector-memory ops this wave issued since its last DMA
    int wv;
    int slot = kRbmSlot;  // bytes per ring slot
    int nw = kRbmWaves;   // waves of the workgroup (they share the DMA pieces)
};

// rows per chunk of a layer with KB k blocks (chunk <= kRbmSlot)
__host__ __device__ constexpr int rbm_rows(int KB) { return KB >= 8 ? 2 : (KB >= 4 ? 4 : 8); }
__host__ __device__ constexpr int rbm_chunk_kb(int KB, int bias = 1) { return rbm_rows(KB) * (2 * KB + bias); }

__device__ __forceinline__ void rbm_dma(RStream& s, int ckb) {
    char* slot = s.lds + ((s.q + 1) & 1) * s.slot;
    const uint32_t l16 = lane16();
    for (int pc = s.wv; pc < ckb; pc += s.nw)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s.src + pc * 1024 + l16),
                                         (__attribute__((address_space(3))) void*)(slot + pc * 1024), 16, 0, 0);
    s.src += ckb * 1024;
    s.nvm = 0;
}

// s_waitcnt vmcnt(min(n, 15)): waiting for fewer outstanding ops than were issued
// after the DMA only waits longer
__device__ __forceinline__ void rbm_wait_vm(int n) {
    switch (n) {
#define NR_VMC(k) \
    case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
        NR_VMC(0) NR_VMC(1) NR_VMC(2) NR_VMC(3) NR_VMC(4) NR_VMC(5) NR_VMC(6) NR_VMC(7)
        NR_VMC(8) NR_VMC(9) NR_VMC(10) NR_VMC(11) NR_VMC(12) NR_VMC(13) NR_VMC(14)
#undef NR_VMC
        default: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    }
}

// chunk boundary: chunk q published to the workgroup, chunk q+1 (next_ckb KB, 0: none) issued
__device__ __forceinline__ void rbm_boundary(RStream& s, int next_ckb) {
    rbm_wait_vm(s.nvm);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (next_ckb > 0) rbm_dma(s, next_ckb);
}

template <int OFF>
__device__ __forceinline__ void rbm_dsr(bf16x8& d, uint32_t a) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "i"(OFF));
}

// s_waitcnt lgkmcnt(N) tied to the registers it publishes
template <int N>
__device__ __forceinline__ void rbm_lgkm_t(bf16x8& a) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N));
}
template <int N>
__device__ __forceinline__ void rbm_lgkm_t(bf16x8& a, bf16x8& b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}

#ifndef NR_RBM_PD
#define NR_RBM_PD 3  // LDS items read ahead of their MFMA
#endif

// One MFMA layer, row-block major.  in(kb): the layer input's block kb (InBlk in
// registers) for kb >= XL; blocks kb < XL are B-operand images in LDS at xaddr
// (the skip layer's x_enc).  fin(rb, acc, bias_frag): epilogue of a finished row
// block, run at MFMA EPI_AT of the next one (the last after the layer).
//
// A chunk is R row blocks.  Its LDS reads form one flat sequence, per row block:
// [its x_enc fragments (XL > 0)][its 2*KB A fragments][its bias fragment], read
// PD items ahead, so the next row block's first fragments are already in flight
// while this one's last MFMAs issue.  Each wait is a counted lgkmcnt tied to the
// registers it publishes (reads complete in order: a wait also covers every
// older item, e.g. the x_enc fragment and the previous bias).
template <int PREC, int KB, int NB, int XL, class In, class Fin, int BIAS = 1>
__device__ __forceinline__ void rbm_layer(RStream& s, int next_ckb, const In& in, Fin& fin, uint32_t xaddr = 0) {
    constexpr int R = rbm_rows(KB);
    constexpr int N = 2 * KB;              // MFMAs per row block
    constexpr int RBK = 2 * KB + BIAS;     // LDS fragments per row block (weights [+ bias])
    constexpr int RBI = 2 * XL + N + BIAS; // read items per row block
    constexpr int T = R * RBI;             // read items per chunk
    constexpr int CKB = R * RBK;
    constexpr int PD = NR_RBM_PD;          // items read ahead
    constexpr int EPI_AT = N >= 8 ? 4 : N / 2;
    static_assert(NB % R == 0 && CKB * 1024 <= kRbmSlot, "row-block chunk");
    f32x16 acc[2];
    bf16x8 bfr[2];
    rbm_static_for<NB / R>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        rbm_boundary(s, c + 1 < NB / R ? CKB : next_ckb);
        const uint32_t slot = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(s.lds)) + (s.q & 1) * s.slot + lane16();
        bf16x8 fa[PD + 1];
        bf16x8 xb[XL > 0 ? 2 * XL : 1];
        auto issue = [&](auto jj) {
            constexpr int j = decltype(jj)::value;
            constexpr int r = j / RBI, f = j % RBI;
            if constexpr (f < 2 * XL)
                rbm_dsr<f * 1024>(xb[f], xaddr);
            else if constexpr (f < 2 * XL + N)
                rbm_dsr<(r * RBK + f - 2 * XL) * 1024>(fa[j % (PD + 1)], slot);
            else
                rbm_dsr<(r * RBK + N) * 1024>(bfr[(c * R + r) & 1], slot);
        };
        rbm_static_for<PD>(issue);
        rbm_static_for<T>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            if constexpr (j + PD < T) issue(std::integral_constant<int, j + PD>{});
            constexpr int r = j / RBI, f = j % RBI, rb = c * R + r;
            if constexpr (f >= 2 * XL && f < 2 * XL + N) {  // an A item: one MFMA
                constexpr int k = f - 2 * XL;
                constexpr int younger = T - 1 - j < PD ? T - 1 - j : PD;
                bf16x8& a = fa[j % (PD + 1)];
                if constexpr (k < 2 * XL)
                    rbm_lgkm_t<younger>(a, xb[k]);  // x_enc items are older than every A item
                else if constexpr (k == 0 && r > 0 && BIAS)
                    rbm_lgkm_t<younger>(a, bfr[(rb - 1) & 1]);  // so is the previous bias
                else
                    rbm_lgkm_t<younger>(a);
                f32x16& ac = acc[rb & 1];
                if constexpr (k == 0) zero(ac);
                if constexpr (k < 2 * XL)
                    ac = mfma16<PREC>(a, xb[k], ac);
                else
                    ac = mfma16<PREC>(a, in(k >> 1).s[k & 1], ac);
                if constexpr (rb > 0 && k == EPI_AT) fin(rb - 1, acc[(rb - 1) & 1], bfr[(rb - 1) & 1]);
            }
        });
        // the chunk's last item is its last row block's bias
        if constexpr (BIAS) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bfr[(c * R + R - 1) & 1]));
        ++s.q;
    });
    fin(NB - 1, acc[(NB - 1) & 1], bfr[(NB - 1) & 1]);
}

// ---- row-block epilogues ----
// trunk layer: bias, 16-bit pack, ReLU on packed pairs, mask bits; training stores the
// block (B-operand image of h_i); the last trunk layer also feeds the sigma head
template <int PREC, bool TRAIN, bool ACT = TRAIN>
struct RbmTrunkFin {
    InBlk<PREC> (&out)[kHB];
    unsigned (&mw)[4];
    char* sv;  // saved image of h_i (training)
    int64_t tile;
    int& nvm;
    bool last;
    float& sg;
    const float* wsig;  // LDS: w_sigma vector image, this lane's half
    __device__ __forceinline__ void operator()(int rb, f32x16& a, const bf16x8& bf) const {
        a = mfma16<PREC>(bf, ones16<PREC>(), a);
        bf16x8 o[2];
        epi16_blk<PREC, true, TRAIN>(a, o, mw, rb);
        out[rb] = InBlk<PREC>{{o[0], o[1]}};
        if constexpr (ACT) {
            store_img<PREC>(sv, tile, kHB, rb, out[rb]);
            nvm += 2;
        }
        // sigma head on the fp32 activations (same FMA chain as the pair-image form)
        if (last)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wsig + rb * 32 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) sg = fmaf(relu_f(a[4 * g + e]), w[e], sg);
            }
    }
};

// feature_linear: bias, 16-bit pack (no activation); training stores feat
template <int PREC, bool ACT>
struct RbmFeatFin {
    InBlk<PREC> (&out)[kHB];
    char* sv;
    int64_t tile;
    int& nvm;
    __device__ __forceinline__ void operator()(int rb, f32x16& a, const bf16x8& bf) const {
        a = mfma16<PREC>(bf, ones16<PREC>(), a);
        bf16x8 o[2];
        unsigned unused[4];
        epi16_blk<PREC, false, false>(a, o, unused, rb);
        out[rb] = InBlk<PREC>{{o[0], o[1]}};
        if constexpr (ACT) {
            store_img<PREC>(sv, tile, kHB, rb, out[rb]);
            nvm += 2;
        }
    }
};

// dir_linear: bias, ReLU in fp32 (the rgb head reads it), pack + mask bits; training
// stores h_c; the three rgb rows accumulate
template <int PREC, bool TRAIN, bool ACT = TRAIN>
struct RbmDirFin {
    unsigned (&mw)[4];
    char* sv;
    int64_t tile;
    int& nvm;
    float (&sc)[3];
    const float* wrgb;  // LDS: the W_rgb row vector images, this lane's half
    __device__ __forceinline__ void operator()(int rb, f32x16& a, const bf16x8& bf) const {
        constexpr int NC = kHB / 2;
        a = mfma16<PREC>(bf, ones16<PREC>(), a);
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = relu_f(a[r]);
        bf16x8 o[2];
        epi16_blk<PREC, false, TRAIN>(a, o, mw, rb);
        if constexpr (ACT) {
            store_img<PREC>(sv, tile, NC, rb, InBlk<PREC>{{o[0], o[1]}});
            nvm += 2;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wrgb + c * NC * 32 + rb * 32 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[c] = fmaf(a[4 * g + e], w[e], sc[c]);
            }
    }
};

template <int PREC, int XB>
__device__ __forceinline__ void rbm_xenc(const PeRev& pr, int L, bool h1, InBlk<PREC> (&xe)[XB]) {
#pragma unroll
    for (int kb = 0; kb < XB; ++kb) {
        f32x16 v;
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = pe_fast(pr, 32 * kb + acc_row(r, 0), 32 * kb + acc_row(r, 1), h1, L);
        to_in<PREC>(v, xe[kb]);
    }
}

// TRAIN: the ReLU masks are built and stored; ACT: so are the activation images (x_enc,
// h_i, feat, d_enc, h_c).  <true, true> is the training forward, <false, false> inference,
// <true, false> the frozen-field forward: masks alone, into a region without padding
// tiles, so a wave past the last tile stores nothing and counts nothing into s.nvm (the
// count is per wave, and so is each stream wait).
template <int PREC, int XB, int DB, bool TRAIN, int W, bool ACT = TRAIN>
__global__ __launch_bounds__(W * 64, 1) void mlp_fwd_rbm_kernel(RbmArgs a) {
    static_assert(W >= 3, "waves 0..2 stage the head weights");
    static_assert(TRAIN || !ACT, "activation images come with the masks");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, ml = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tiles past the end run on zero inputs; their stores land in the 16-tile
    // padding of the saved images (make_sizes), so every wave issues the same ops
    const int64_t tile = static_cast<int64_t>(blockIdx.x) * W + wv;
    const int64_t m = tile * 32 + ml;
    const bool valid = m < a.M;
    const int n = a.n_layers;
    u32x4* masks = reinterpret_cast<u32x4*>(a.saved + a.mask_off);
    char* xlds = lds + rbm_xenc_off() + wv * XB * 2 * kFragBytes;  // this wave's x_enc image
    const float* hl = reinterpret_cast<const float*>(lds + rbm_head_off(XB, W)) + 16 * h;

    // head weights -> LDS (3 KB, LDS-DMA by waves 0..2; published with chunk 0)
    if (wv < 3)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(a.packed + a.vhead + wv * 1024 + lane16()),
            (__attribute__((address_space(3))) void*)(lds + rbm_head_off(XB, W) + wv * 1024), 16, 0, 0);

    // x_enc: layer 0's input in registers, the skip layer's from LDS
    InBlk<PREC> xe[XB];
    {
        const float x0 = valid ? a.x[3 * m] : 0.f, x1 = valid ? a.x[3 * m + 1] : 0.f,
                    x2 = valid ? a.x[3 * m + 2] : 0.f;
        rbm_xenc<PREC, XB>(pe_rev(x0, x1, x2), a.L, h != 0, xe);
    }
#pragma unroll
    for (int kb = 0; kb < XB; ++kb) {
        *reinterpret_cast<bf16x8*>(xlds + (2 * kb) * kFragBytes + lane16()) = xe[kb].s[0];
        *reinterpret_cast<bf16x8*>(xlds + (2 * kb + 1) * kFragBytes + lane16()) = xe[kb].s[1];
        if constexpr (ACT) store_img<PREC>(a.saved + a.sv_off[SV_XENC], tile, XB, kb, xe[kb]);
    }

    RStream s{lds, a.packed + a.base, -1, 0, wv, kRbmSlot, W};
    rbm_dma(s, rbm_chunk_kb(XB));
    s.q = 0;

    constexpr int CK_H = rbm_chunk_kb(kHB), CK_SKIP = rbm_chunk_kb(XB + kHB);
    auto ckb_of = [&](int i) {  // first chunk of trunk layer i (i == n: the feature layer)
        return (i < n && i > 0 && ((a.skips >> (i - 1)) & 1u)) ? CK_SKIP : CK_H;
    };

    InBlk<PREC> hA[kHB], hB[kHB];
    unsigned mw[4];
    float sg = 0.f;
    const uint32_t xaddr = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(xlds)) + lane16();

    auto trunk = [&](int i, const auto& in, InBlk<PREC>(&hout)[kHB], auto kbc, auto xlc) {
        constexpr int KBL = decltype(kbc)::value, XL = decltype(xlc)::value;
#pragma unroll
        for (int q = 0; q < 4; ++q) mw[q] = 0u;
        RbmTrunkFin<PREC, TRAIN, ACT> fin{hout, mw, ACT ? a.saved + a.sv_off[SV_H0 + i] : nullptr, tile, s.nvm,
                                          i == n - 1, sg, hl};
        rbm_layer<PREC, KBL, kHB, XL>(s, ckb_of(i + 1), in, fin, xaddr);
        if constexpr (TRAIN) {
            if (ACT || tile < a.tiles) {  // wave-uniform
                masks[(tile * a.n_mask + i) * 64 + lane] = u32x4{mw[0], mw[1], mw[2], mw[3]};
                s.nvm += 1;
            }
        }
    };
    // trunk layer i (i >= 1) from hin into hout: plain, or [x_enc, h] after a skip
    auto trunk_any = [&](int i, InBlk<PREC>(&hin)[kHB], InBlk<PREC>(&hout)[kHB]) {
        if ((a.skips >> (i - 1)) & 1u) {
            auto in = [&](int kb) -> const InBlk<PREC>& { return hin[kb >= XB ? kb - XB : 0]; };
            trunk(i, in, hout, std::integral_constant<int, XB + kHB>{}, std::integral_constant<int, XB>{});
        } else {
            auto in = [&](int kb) -> const InBlk<PREC>& { return hin[kb]; };
            trunk(i, in, hout, std::integral_constant<int, kHB>{}, std::integral_constant<int, 0>{});
        }
    };

    {
        auto in = [&](int kb) -> const InBlk<PREC>& { return xe[kb]; };
        trunk(0, in, hA, std::integral_constant<int, XB>{}, std::integral_constant<int, 0>{});
    }
    for (int i = 1; i < n; i += 2) {
        trunk_any(i, hA, hB);
        if (i + 1 == n) {
#pragma unroll
            for (int b = 0; b < kHB; ++b) hA[b] = hB[b];
            break;
        }
        trunk_any(i + 1, hB, hA);
    }

    // this tile's directions, in flight over the feature layer
    float pd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pd[c] = (DB > 0 && valid) ? a.d[3 * m + c] : 0.f;

    // feature_linear: h_{n-1} (hA) -> feat (hB)
    {
        RbmFeatFin<PREC, ACT> fin{hB, ACT ? a.saved + a.sv_off[a.sv_feat] : nullptr, tile, s.nvm};
        auto in = [&](int kb) -> const InBlk<PREC>& { return hA[kb]; };
        rbm_layer<PREC, kHB, kHB, 0>(s, rbm_chunk_kb(kHB + DB), in, fin);
    }
    // dir_linear over [feat, d_enc]
    InBlk<PREC> de[DB > 0 ? DB : 1];
    if constexpr (DB > 0) {
        const PeRev pr = pe_rev(pd[0], pd[1], pd[2]);
#pragma unroll
        for (int kb = 0; kb < DB; ++kb) {
            f32x16 v;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                v[r] = pe_fast(pr, 32 * kb + acc_row(r, 0), 32 * kb + acc_row(r, 1), h != 0, a.Ld);
            to_in<PREC>(v, de[kb]);
            if constexpr (ACT) {
                store_img<PREC>(a.saved + a.sv_off[a.sv_denc], tile, DB, kb, de[kb]);
                s.nvm += 2;
            }
        }
    }
    float sc[3] = {0.f, 0.f, 0.f};
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) mw[q] = 0u;
        RbmDirFin<PREC, TRAIN, ACT> fin{mw, ACT ? a.saved + a.sv_off[a.sv_hc] : nullptr, tile, s.nvm, sc, hl + 256};
        auto in = [&](int kb) -> const InBlk<PREC>& { return kb < kHB ? hB[kb] : de[kb >= kHB ? kb - kHB : 0]; };
        rbm_layer<PREC, kHB + DB, kHB / 2, 0>(s, 0, in, fin);
        if constexpr (TRAIN)
            if (ACT || tile < a.tiles) masks[(tile * a.n_mask + n) * 64 + lane] = u32x4{mw[0], mw[1], mw[2], mw[3]};
    }

    // heads: sigma = relu(w_sigma . h_{n-1} + b), rgb = sigmoid(W_rgb h_c + b)
    float sp = sg + __shfl_xor(sg, 32);
    sp = sp + a.params[a.sig_b];
    sp = sp > 0.f ? sp : 0.f;
    float pr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = sc[c] + __shfl_xor(sc[c], 32);
        v = v + a.params[a.rgb_b + c];
        pr[c] = 1.0f / (1.0f + expf(-v));
    }
    if (valid && h == 0) {
        a.rgb[3 * m] = pr[0];
        a.rgb[3 * m + 1] = pr[1];
        a.rgb[3 * m + 2] = pr[2];
        a.sigma[m] = sp;
    }
}

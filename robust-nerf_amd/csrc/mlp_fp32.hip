// fp32 parity mode of the fused NeRF MLP: forward and backward dX chain, CHUNK-MAJOR.
// Reference: noisy_src/model.py:145-196 (NeRF.forward) and its autograd backward.
//
// The layer images are chunk-major (a chunk = all row blocks of one k block, fp32
// 32x32x2 MFMA, k-step t: lane half h <-> input feature (t&3) + 8(t>>2) + 4h) and are
// streamed through an LDS double buffer shared by the workgroup's 4 waves; each wave
// owns one 32-sample tile and keeps its activations in registers as fp32 B operands
// (an accumulator tile is the next layer's B operand as it is).  256 threads per
// workgroup: one wave per SIMD, with the full 512-register budget.
#include "mlp_dev.hpp"
#include "mlp_launch.hpp"

namespace nr {

constexpr int kNT = 256;            // threads per workgroup
// 32-sample tiles per wave.  The kernels keep their loops over a wave's tiles: with
// the single-trip loops written out the compiler allocates registers differently.
constexpr int TPW = 1;
constexpr int kFP = NR_PREC_FP32;
typedef InBlk<kFP> Blk;             // one 32-feature block of a tile: the accumulator registers
constexpr int kFPB32 = kFPB<kFP>;   // 1-KB fragments per 32x32 block

// bias + optional ReLU on NBO blocks; mask bits (bit (nb&1)*16+r of word nb>>1) into w[4].
template <int NBO, bool RELU>
__device__ __forceinline__ void bias_act(f32x16 (&acc)[NBO], const VImg& bias, unsigned (&w)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = 0u;
#pragma unroll
    for (int nb = 0; nb < NBO; ++nb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b = NR_VEC(bias, nb, g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                float v = acc[nb][r] + b[e];
                if (RELU) v = v > 0.f ? v : 0.f;
                acc[nb][r] = v;
                w[nb >> 1] |= (v > 0.f ? 1u : 0u) << ((nb & 1) * 16 + r);
            }
        }
    }
}

// ------------------------------------------------------ weight stream -----
// A sequence of chunks (StreamDesc) consumed in order through an LDS double buffer,
// staged one chunk ahead by LDS-DMA: load(q+1) is issued before chunk q's MFMAs and
// waited for after them, then one barrier.  The slot written at step q was last read
// at step q-1, which every wave finished before the previous barrier.
struct Ring {
    char* lds;
    int slot_bytes;
    int q;                         // chunk in the current slot
    const char* src;               // next chunk to load
    int wv;                        // wave index in the workgroup (wave-uniform)
};

#ifndef NR_APF
#define NR_APF 3  // > 0: the A fragments of row block r + 1 are read (asm) while row block r multiplies; 0: plain loads
#endif

// LDS-DMA staging: chunk q goes straight into its slot (no registers); the barrier
// that publishes it is preceded by a vmcnt wait.
struct Stager {
    __device__ __forceinline__ void load(Ring& ring, const StreamDesc& sd, int q) {
        if (q >= sd.nq) return;
        load_sized(ring, q, sd.ckb[q], sd.cadv[q]);
    }
    // chunk q of ckb KB (advance cadv KB): sizes from the caller, no scalar loads
    __device__ __forceinline__ void load_sized(Ring& ring, int q, int ckb, int cadv) {
        const int bytes = ckb * 1024;
        char* slot = ring.lds + (q & 1) * ring.slot_bytes;
        const uint32_t l16 = lane16();
        for (int pc = ring.wv; pc * 1024 < bytes; pc += kNT / 64)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(ring.src + pc * 1024 + l16),
                (__attribute__((address_space(3))) void*)(slot + pc * 1024), 16, 0, 0);
        ring.src += cadv * 1024;
    }

    // Wait for this wave's pieces of the next chunk only: the `after` vector-memory
    // ops issued since (the chunk's saved-activation stores) may stay in flight
    // across the barrier (vmcnt retires in issue order).
    __device__ __forceinline__ void wait(int after = 0) {
        switch (after) {
            case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
    }
};

// A wave's activation storage: NBLK 32-feature blocks of each of its tiles, in registers.
template <int NBLK>
struct Act {
    Blk v[TPW][NBLK];
    __device__ __forceinline__ Blk operator()(int t, int kb) const { return v[t][kb]; }
    __device__ __forceinline__ void put(int t, int nb, const Blk& x) { v[t][nb] = x; }
};

// Saves each B operand a forward stream consumes (= the previous layer's output block
// kb) as its B-operand image, one block per chunk: the saved-activation stores spread
// over the stream instead of bursting at every layer end.
struct Sink {
    char* region;  // nullptr: no store
    int nblk;
    int64_t tile0;
    unsigned tok;  // bit t: tile t exists
    __device__ __forceinline__ void operator()(int t, int kb, const Blk& v) const {
        if (region != nullptr && ((tok >> t) & 1u)) store_img(region, tile0 + t, nblk, kb, v);
    }
    // vector-memory stores one chunk issues (wave-uniform)
    __device__ __forceinline__ int stores() const {
        return region == nullptr ? 0 : kFPB32 * __builtin_popcount(tok & ((1u << TPW) - 1u));
    }
};

// Workgroup barrier of the weight stream.  Not __syncthreads(): its release fence
// would also drain every in-flight global store (vmcnt(0)) at every chunk.  This
// wave's reads of the slot about to be refilled complete first (lgkmcnt(0)); LDS-DMA
// completion is the stager's counted vmcnt.
__device__ __forceinline__ void stream_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// A operands: the four 1-KB fragments of one row block, read by asm, and the counted
// wait that publishes one of them (n: the reads issued after it, all younger LDS
// reads; SMEM only ever makes this wait longer).  Plain loads here get sunk by the
// compiler next to their use: one read, lgkmcnt(0), one MFMA, every time.
__device__ __forceinline__ void ds_read_quad(f32x4 (&dst)[4], uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1" : "=v"(dst[0]) : "v"(addr));
    asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(dst[1]) : "v"(addr));
    asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(dst[2]) : "v"(addr));
    asm volatile("ds_read_b128 %0, %1 offset:3072" : "=v"(dst[3]) : "v"(addr));
}
__device__ __forceinline__ void lgkm_wait_one(int n, f32x4& a) {
    switch (n) {
        case 0: asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)); break;
        case 1: asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(a)); break;
        case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(a)); break;
        case 3: asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(a)); break;
        case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a)); break;
        case 5: asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(a)); break;
        case 6: asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(a)); break;
        default: asm volatile("s_waitcnt lgkmcnt(7)" : "+v"(a)); break;
    }
}

// acc1[t][r] += A(row block nb0 + r) . in[t]   (r < N1)
// acc2[t][r] += A(row block nb0 + N1 + r) . in[t]   (r < N2)
// over KBN consecutive stream chunks (k blocks); in[t] = src(t, kb), handed to the sink.
template <int N1, int N2, int KBN, class Src>
__device__ __forceinline__ void stream_gemm(f32x16 (&acc1)[TPW][N1 > 0 ? N1 : 1],
                                            f32x16 (&acc2)[TPW][N2 > 0 ? N2 : 1], int nb0, const Src& src,
                                            Ring& ring, Stager& st, const StreamDesc& sd,
                                            const Sink& sink = Sink{nullptr, 0, 0, 0u}) {
    // Chunk sizes, read once per segment: every chunk of a segment has this
    // segment's size; the prefetch in its last step is the next segment's first chunk.
    const int q0 = ring.q;
    const int ckb_this = sd.ckb[q0], adv_this = sd.cadv[q0];
    const bool has_next = q0 + KBN < sd.nq;
    const int ckb_next = has_next ? sd.ckb[q0 + KBN] : 0, adv_next = has_next ? sd.cadv[q0 + KBN] : 0;
#pragma unroll
    for (int kb = 0; kb < KBN; ++kb) {
        if (kb < KBN - 1)
            st.load_sized(ring, ring.q + 1, ckb_this, adv_this);
        else if (has_next)
            st.load_sized(ring, ring.q + 1, ckb_next, adv_next);
        asm volatile("" ::: "memory");  // the sink stores below stay younger than the DMA
        const char* slot = ring.lds + (ring.q & 1) * ring.slot_bytes + lane16();
        Blk in[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) in[t] = src(t, kb);
        constexpr int NRB = N1 + N2;
        const uint32_t abase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(slot)) +
                               static_cast<uint32_t>(nb0 * kFPB32 * kFragBytes);
        f32x4 aq[2][4];  // row block r + 1 is read while row block r multiplies
        if constexpr (NR_APF > 0) ds_read_quad(aq[0], abase);
#pragma unroll
        for (int t = 0; t < TPW; ++t) sink(t, kb, in[t]);
#pragma unroll
        for (int r = 0; r < NRB; ++r) {
            const char* fp = slot + (nb0 + r) * kFPB32 * kFragBytes;
            constexpr int I2 = N2 > 0 ? N2 : 1;
            const int r1 = r < N1 ? r : 0;
            const int r2 = r >= N1 ? (r - N1) % I2 : 0;
            if constexpr (NR_APF > 0)
                if (r + 1 < NRB) ds_read_quad(aq[(r + 1) & 1], abase + (r + 1) * 4 * kFragBytes);
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                f32x4 a;
                if constexpr (NR_APF > 0) {
                    a = aq[r & 1][tq];
                    lgkm_wait_one((r + 1 < NRB ? 4 : 0) + 3 - tq, a);
                } else {
                    a = *reinterpret_cast<const f32x4*>(fp + tq * kFragBytes);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < TPW; ++t) {
                        if (r < N1)
                            acc1[t][r1] = mfma_f32(a[e], in[t].v[4 * tq + e], acc1[t][r1]);
                        else
                            acc2[t][r2] = mfma_f32(a[e], in[t].v[4 * tq + e], acc2[t][r2]);
                    }
            }
        }
        st.wait(sink.stores());
        stream_barrier();
        ++ring.q;
    }
}

__device__ __forceinline__ void stream_begin(Ring& ring, Stager& st, const char* __restrict__ packed,
                                             const StreamDesc& sd) {
    ring.q = 0;
    ring.src = packed + sd.base;
    st.load(ring, sd, 0);
    st.wait();
    __syncthreads();
}

// ------------------------------------------------------------ forward -----
template <int XB, int DB, bool TRAIN>
__global__ __launch_bounds__(kNT, 1) void mlp_fwd_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, ml = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tile0 = (static_cast<int64_t>(blockIdx.x) * (kNT / 64) + wv) * TPW;
    const int n = a.n_layers;
    float px[TPW][3];
    bool tok[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int64_t m = (tile0 + t) * 32 + ml;
        tok[t] = tile0 + t < a.tiles;
        const bool valid = m < a.M;
        px[t][0] = valid ? a.x[3 * m] : 0.f;
        px[t][1] = valid ? a.x[3 * m + 1] : 0.f;
        px[t][2] = valid ? a.x[3 * m + 2] : 0.f;
    }
    u32x4* masks = reinterpret_cast<u32x4*>(a.saved + a.mask_off);
    unsigned tokm = 0u;
#pragma unroll
    for (int t = 0; t < TPW; ++t) tokm |= (tok[t] ? 1u : 0u) << t;
    // training saves each layer input as the next stream consumes it
    auto sink_of = [&](int sv, int nblk) {
        return Sink{TRAIN ? a.saved + a.sv_off[sv] : nullptr, nblk, tile0, tokm};
    };

    Ring ring{lds, a.slot_bytes, 0, nullptr, wv};
    Stager st;
    stream_begin(ring, st, a.packed, a.sd);

    f32x16 acc[TPW][kHB];
    Act<kHB> hin;
    f32x16 dummy[TPW][1];
    unsigned w[TPW][4];
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int nb = 0; nb < kHB; ++nb) zero(acc[t][nb]);
        const bool skip_in = i > 0 && ((a.skips >> (i - 1)) & 1u);
        if (i == 0 || skip_in) {
            // x_enc is not kept in registers: the skip layer reloads the saved
            // copy (training) or recomputes it (inference)
            Act<XB> xe;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                if (TRAIN && i > 0) {
#pragma unroll
                    for (int kb = 0; kb < XB; ++kb) {
                        if (tok[t])
                            load_img(a.saved + a.sv_off[SV_XENC], tile0 + t, XB, kb, xe.v[t][kb]);
                        else
                            xe.v[t][kb] = Blk{};
                    }
                    continue;
                }
                // opaque copy: keeps the encoding from being hoisted out of the
                // layer loop (and spilled) as a loop invariant
                float p0 = px[t][0], p1 = px[t][1], p2 = px[t][2];
                asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2));
#pragma unroll
                for (int kb = 0; kb < XB; ++kb) {
                    f32x16 v;
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = pe_feat(p0, p1, p2, 32 * kb + acc_row(r, h), a.L);
                    Blk o;
                    to_in(v, o);
                    if constexpr (TRAIN)
                        if (tok[t]) store_img(a.saved + a.sv_off[SV_XENC], tile0 + t, XB, kb, o);
                    // constant indices: the body (accurate sinf) is too big for the
                    // pragma to unroll, and a run-time index put xe in scratch, whose
                    // reloads in the stream then drained the in-flight weight DMA
#pragma unroll
                    for (int k2 = 0; k2 < XB; ++k2)
                        if (k2 == kb) xe.v[t][k2] = o;
                }
            }
            stream_gemm<kHB, 0, XB>(acc, dummy, 0, xe, ring, st, a.sd);
        }
        if (i > 0) stream_gemm<kHB, 0, kHB>(acc, dummy, 0, hin, ring, st, a.sd, sink_of(SV_H0 + i - 1, kHB));
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            bias_act<kHB, true>(acc[t], vimg(a.packed, a.vb[i], lane), w[t]);
#pragma unroll
            for (int nb = 0; nb < kHB; ++nb) {
                Blk v;
                to_in(acc[t][nb], v);
                hin.put(t, nb, v);
            }
            if constexpr (TRAIN)
                if (tok[t]) masks[((tile0 + t) * a.n_mask + i) * 64 + lane] = u32x4{w[t][0], w[t][1], w[t][2], w[t][3]};
        }
    }

    // sigma head (VALU): relu(w_sigma . h + b), from the fp32 activations
    float sp[TPW];
    {
        const PImg ws = pimg(a.packed, a.vsig);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            f32x2 s2 = {0.f, 0.f};
#pragma unroll
            for (int nb = 0; nb < kHB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s2 = __builtin_elementwise_fma(bcast2(relu_f(acc[t][nb][r])), ws.at(nb, r), s2);
            sp[t] = h ? s2[1] : s2[0];
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            sp[t] += __shfl_xor(sp[t], 32);
            sp[t] = sp[t] + a.params[a.sig_b];
            sp[t] = sp[t] > 0.f ? sp[t] : 0.f;
        }
    }

    // feature_linear (no activation)
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) zero(acc[t][nb]);
    stream_gemm<kHB, 0, kHB>(acc, dummy, 0, hin, ring, st, a.sd, sink_of(SV_H0 + n - 1, kHB));
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        bias_act<kHB, false>(acc[t], vimg(a.packed, a.vb[n], lane), w[t]);
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) {
            Blk v;
            to_in(acc[t][nb], v);
            hin.put(t, nb, v);
        }
    }

    // dir_linear over [feat, d_enc], ReLU
    constexpr int NC = kHB / 2;
    f32x16 ac[TPW][NC];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int nb = 0; nb < NC; ++nb) zero(ac[t][nb]);
    stream_gemm<NC, 0, kHB>(ac, dummy, 0, hin, ring, st, a.sd, sink_of(a.sv_feat, kHB));
    if constexpr (DB > 0) {
        Act<DB> de;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int64_t m = (tile0 + t) * 32 + ml;
            const bool valid = m < a.M;
            const float d0 = valid ? a.d[3 * m] : 0.f, d1 = valid ? a.d[3 * m + 1] : 0.f,
                        d2 = valid ? a.d[3 * m + 2] : 0.f;
#pragma unroll
            for (int kb = 0; kb < DB; ++kb) {
                f32x16 v;
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = pe_feat(d0, d1, d2, 32 * kb + acc_row(r, h), a.Ld);
                to_in(v, de.v[t][kb]);
                if constexpr (TRAIN)
                    if (tok[t]) store_img(a.saved + a.sv_off[a.sv_denc], tile0 + t, DB, kb, de.v[t][kb]);
            }
        }
        stream_gemm<NC, 0, DB>(ac, dummy, 0, de, ring, st, a.sd);
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        bias_act<NC, true>(ac[t], vimg(a.packed, a.vb[n + 1], lane), w[t]);
        if constexpr (TRAIN) {
            if (tok[t]) {
#pragma unroll
                for (int nb = 0; nb < NC; ++nb) {
                    Blk v;
                    to_in(ac[t][nb], v);
                    store_img(a.saved + a.sv_off[a.sv_hc], tile0 + t, NC, nb, v);
                }
                masks[((tile0 + t) * a.n_mask + n) * 64 + lane] = u32x4{w[t][0], w[t][1], w[t][2], w[t][3]};
            }
        }
        // rgb head (VALU): sigmoid(W_rgb h_c + b)
        float pr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const PImg wr = pimg(a.packed, a.vrgb + c * NC * 128);
            f32x2 s2 = {0.f, 0.f};
#pragma unroll
            for (int nb = 0; nb < NC; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s2 = __builtin_elementwise_fma(bcast2(ac[t][nb][r]), wr.at(nb, r), s2);
            float s = h ? s2[1] : s2[0];
            s += __shfl_xor(s, 32);
            s = s + a.params[a.rgb_b + c];
            pr[c] = 1.0f / (1.0f + expf(-s));
        }
        const int64_t m = (tile0 + t) * 32 + ml;
        if (m < a.M && h == 0) {
            a.rgb[3 * m] = pr[0];
            a.rgb[3 * m + 1] = pr[1];
            a.rgb[3 * m + 2] = pr[2];
            a.sigma[m] = sp[t];
        }
    }
}

// ----------------------------------------------------------- backward -----
// WANT_X: the input-gradient variant, which also carries d x_enc through the trunk.
// Every dz is stored as soon as it is formed (storing each while the next stream
// consumes it measured slower: 1.50 vs 1.35 ms).
template <int XB, int DB, bool WANT_X>
__global__ __launch_bounds__(kNT, 1) void mlp_bwd_kernel(BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, ml = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // wave -> its tile (select_tile); waves without one run on zero inputs and store nothing
    static_assert(TPW == 1, "the active-tile selection gives each wave one tile");
    const TileSel ts = select_tile(a.flags, a.blk_count, a.nseg, a.tiles, kNT / 64, wv);
    if (ts.idle) {  // workgroup-uniform
        finish_tiles(ts, a.nseg, a.tiles, a.dw_list, a.count);
        return;
    }
    const bool live = ts.live;
    const int64_t tile0 = live ? ts.tile : 0;
    const int n = a.n_layers;
    const u32x4* masks = reinterpret_cast<const u32x4*>(a.saved + a.mask_off);
    bool tok[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) tok[t] = live;
    auto store_dz = [&](int wsid, int nblk, int t, int nb, const Blk& v) {
        if (tok[t]) store_img(a.ws + a.ws_off[wsid], tile0 + t, nblk, nb, v);
    };
    auto mask_of = [&](int t, int layer) -> u32x4 {
        return tok[t] ? masks[((tile0 + t) * a.n_mask + layer) * 64 + lane] : u32x4{0u, 0u, 0u, 0u};
    };

    Ring ring{lds, a.slot_bytes, 0, nullptr, wv};
    Stager st;
    stream_begin(ring, st, a.packed, a.sd);

    // heads: sigmoid / relu backward (torch: g * (1 - y) * y ; g * (y > 0))
    constexpr int NC = kHB / 2;
    float dzs[TPW];
    Act<NC> cin;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int64_t m = (tile0 + t) * 32 + ml;
        float dr[3] = {0.f, 0.f, 0.f};
        dzs[t] = 0.f;
        head_grads(a.rgb, a.sigma, a.g_rgb, a.g_sigma, a.gscale, m, tok[t] && m < a.M, dr, dzs[t]);
        if (tok[t]) store_img(a.ws + a.ws_off[a.ws_heads], tile0 + t, 1, 0, heads_blk<kFP>(h, dzs[t], dr));
        // dz_c = (W_rgb^T dz_rgb) * [h_c > 0]  (the rows are written out here and in
        // mlp_bwd_rbm_kernel: through a shared helper this kernel's SGPR spills change)
        f32x16 dc[NC];
        const PImg wr0 = pimg(a.packed, a.vrgb), wr1 = pimg(a.packed, a.vrgb + NC * 128),
                   wr2 = pimg(a.packed, a.vrgb + 2 * NC * 128);
#pragma unroll
        for (int nb = 0; nb < NC; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                f32x2 v = wr0.at(nb, r) * bcast2(dr[0]);
                v = __builtin_elementwise_fma(wr1.at(nb, r), bcast2(dr[1]), v);
                v = __builtin_elementwise_fma(wr2.at(nb, r), bcast2(dr[2]), v);
                dc[nb][r] = h ? v[1] : v[0];
            }
        const u32x4 mwc = mask_of(t, n);
#pragma unroll
        for (int nb = 0; nb < NC; ++nb) {
            to_in_masked(dc[nb], mwc, nb, cin.v[t][nb]);
            store_dz(a.ws_dir, NC, t, nb, cin.v[t][nb]);
        }
    }

    // d [feat | d_enc] = W_dir^T dz_c   (feature_linear has no activation: dz_feat = d feat)
    f32x16 acc[TPW][kHB];
    Act<kHB> hin;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) zero(acc[t][nb]);
    constexpr int DBX = (WANT_X && DB > 0) ? DB : 0;
    f32x16 dd[TPW][DBX > 0 ? DBX : 1];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int k = 0; k < (DBX > 0 ? DBX : 1); ++k) zero(dd[t][k]);
    stream_gemm<kHB, DBX, NC>(acc, dd, 0, cin, ring, st, a.sd);
    if constexpr (DBX > 0) {
        if (a.g_d) {
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int64_t m = (tile0 + t) * 32 + ml;
                const bool valid = tok[t] && m < a.M;
                const float d0 = valid ? a.d[3 * m] : 0.f, d1 = valid ? a.d[3 * m + 1] : 0.f,
                            d2 = valid ? a.d[3 * m + 2] : 0.f;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int kb = 0; kb < DBX; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        pe_feat_bwd(d0, d1, d2, 32 * kb + acc_row(r, h), a.Ld, dd[t][kb][r], g0, g1, g2);
                store_input_grad(a.g_d, m, valid && h == 0, a.inv_gscale, g0, g1, g2);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) {
            Blk v;
            to_in(acc[t][nb], v);
            hin.put(t, nb, v);
            store_dz(a.ws_feat, kHB, t, nb, v);
        }

    // d h_{n-1} = W_feat^T dz_feat + w_sigma dz_sigma, then * [h_{n-1} > 0]
    f32x16 dummy[TPW][1];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) zero(acc[t][nb]);
    // the ReLU masks this stream's output needs are loaded before it (the stream's
    // asm barriers keep loads from being hoisted over it by the compiler)
    u32x4 mwf[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) mwf[t] = mask_of(t, n - 1);
    stream_gemm<kHB, 0, kHB>(acc, dummy, 0, hin, ring, st, a.sd);
    {
        const PImg ws = pimg(a.packed, a.vsig);
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    const f32x2 v = __builtin_elementwise_fma(ws.at(nb, r), bcast2(dzs[t]), bcast2(acc[t][nb][r]));
                    acc[t][nb][r] = h ? v[1] : v[0];
                }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
#pragma unroll
        for (int nb = 0; nb < kHB; ++nb) {
            Blk v;
            to_in_masked(acc[t][nb], mwf[t], nb, v);
            hin.put(t, nb, v);
            store_dz(WS_DZ0 + n - 1, kHB, t, nb, v);
        }
    }

    // trunk: dz_{i-1} = (W_i^T dz_i)[h rows] * [h_{i-1} > 0]; x_enc rows feed g_x
    constexpr int XBX = WANT_X ? XB : 0;
    f32x16 dxe[TPW][XBX > 0 ? XBX : 1];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int k = 0; k < (XBX > 0 ? XBX : 1); ++k) zero(dxe[t][k]);
    for (int i = n - 1; i >= 1; --i) {
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int nb = 0; nb < kHB; ++nb) zero(acc[t][nb]);
        u32x4 mwt[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) mwt[t] = mask_of(t, i - 1);
        if ((a.skips >> (i - 1)) & 1u) {
            // W^T row blocks of a skip layer are [h (8) | x_enc (XB)]; without g_x
            // only the h rows are streamed
            if constexpr (XBX > 0)
                stream_gemm<kHB, XBX, kHB>(acc, dxe, 0, hin, ring, st, a.sd);
            else
                stream_gemm<kHB, 0, kHB>(acc, dummy, 0, hin, ring, st, a.sd);
        } else {
            stream_gemm<kHB, 0, kHB>(acc, dummy, 0, hin, ring, st, a.sd);
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
            for (int nb = 0; nb < kHB; ++nb) {
                Blk v;
                to_in_masked(acc[t][nb], mwt[t], nb, v);
                hin.put(t, nb, v);
                store_dz(WS_DZ0 + i - 1, kHB, t, nb, v);
            }
        }
    }
    if constexpr (XBX > 0) {
        stream_gemm<XBX, 0, kHB>(dxe, dummy, 0, hin, ring, st, a.sd);
        if (a.g_x) {
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int64_t m = (tile0 + t) * 32 + ml;
                const bool valid = tok[t] && m < a.M;
                const float x0 = valid ? a.x[3 * m] : 0.f, x1 = valid ? a.x[3 * m + 1] : 0.f,
                            x2 = valid ? a.x[3 * m + 2] : 0.f;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
                for (int kb = 0; kb < XBX; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        pe_feat_bwd(x0, x1, x2, 32 * kb + acc_row(r, h), a.L, dxe[t][kb][r], g0, g1, g2);
                // store_input_grad's lines, written out: through the helper the XB = 1, DB = 0
                // instance's SGPR spill count changes (profiles/mlp_args_kernel_compare.md)
                g0 += __shfl_xor(g0, 32);
                g1 += __shfl_xor(g1, 32);
                g2 += __shfl_xor(g2, 32);
                if (valid && h == 0) {
                    a.g_x[3 * m] = g0 * a.inv_gscale;
                    a.g_x[3 * m + 1] = g1 * a.inv_gscale;
                    a.g_x[3 * m + 2] = g2 * a.inv_gscale;
                }
            }
        }
    }
    finish_tiles(ts, a.nseg, a.tiles, a.dw_list, a.count);
}

// ----------------------------------------------------------- launchers -----
int launch_fwd(const MlpPlan& p, const FwdArgs& a, bool train, hipStream_t s) {
    // the stream's two LDS slots (fwd_stream, mlp_plan.hpp)
    const size_t lds = 2 * static_cast<size_t>(a.slot_bytes);
    const dim3 grid(static_cast<unsigned>(ceil_div_ll(a.tiles, kNT / 64))), block(kNT);
    const bool found = dispatch_model(p, [&](auto xb, auto db) {
        constexpr int XB = decltype(xb)::value, DB = decltype(db)::value;
        if (train)
            hipLaunchKernelGGL((mlp_fwd_kernel<XB, DB, true>), grid, block, lds, s, a);
        else
            hipLaunchKernelGGL((mlp_fwd_kernel<XB, DB, false>), grid, block, lds, s, a);
    });
    if (!found) {
        set_error("nr_mlp_forward: no kernel instance for XB=%d DB=%d", p.XB, p.DB);
        return NR_EARG;
    }
    return check_launch("nr_mlp_forward");
}

int launch_bwd(const MlpPlan& p, const BwdArgs& a, bool want_x, hipStream_t s) {
    const size_t lds = 2 * static_cast<size_t>(a.slot_bytes);
    // every part of every segment (select_tile's workgroup mapping)
    const dim3 grid(static_cast<unsigned>(a.nseg * (kSegTiles / (kNT / 64)))), block(kNT);
    const bool found = dispatch_model(p, [&](auto xb, auto db) {
        constexpr int XB = decltype(xb)::value, DB = decltype(db)::value;
        if (want_x)
            hipLaunchKernelGGL((mlp_bwd_kernel<XB, DB, true>), grid, block, lds, s, a);
        else
            hipLaunchKernelGGL((mlp_bwd_kernel<XB, DB, false>), grid, block, lds, s, a);
    });
    if (!found) {
        set_error("nr_mlp_backward_dx: no kernel instance for XB=%d DB=%d", p.XB, p.DB);
        return NR_EARG;
    }
    return check_launch("nr_mlp_backward_dx");
}

}  // namespace nr

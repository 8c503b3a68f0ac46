// Backward over the stored B-operand images, all precisions: the active-tile flags
// (tile_flags_kernel), the dW GEMM (mlp_dw_kernel) and its deterministic split-M
// reduction (mlp_dw_reduce_kernel).
//
// The dW GEMM reduces over samples, i.e. over the lanes of the saved-activation and dz
// images; it stages whole tiles in LDS (LDS-DMA) and rebuilds sample-major operands
// with the gfx950 transpose read ds_read_b64_tr_b16 (16-bit) or strided ds_read_b32
// (fp32).
#include "mlp_dev.hpp"
#include "mlp_launch.hpp"

namespace nr {

// ----------------------------------------------------- active tiles ----
// The backward's work list.  A sample whose sigma is exactly 0 (alpha = w = 0, and
// ReLU'(0) = 0 on sigma: reference rendering.py:83) or whose transmittance has
// underflowed to 0 (the cumprod of 1 - alpha + 1e-10, rendering.py:87-96) receives
// exactly zero g_rgb and g_sigma, so every layer's dz for it is zero.  A 32-sample
// tile of such samples only adds exact zeros to dW, so the dX chain, the dW GEMM and
// the input gradients run over the tiles with ANY nonzero incoming gradient (computed
// from the values, never assumed).  One launch, no global scan: the tiles form
// segments of kSegTiles; the launch writes one flag byte per tile and the active count
// of every 64-tile block.  The dX workgroups pick their tiles from those (select_tile:
// the dense order when every tile is active, else eight (four) of a segment's active
// tiles found by a wave scan of its 256 flag bytes), and the segments' leaders
// concatenate them into the dW kernel's list (place_segment), which that kernel splits
// evenly over its chunks.  With every tile active, each kernel sees exactly the dense
// form's tiles in order.
constexpr int kTileFlagThreads = 256;  // 4 waves x 16 tiles: one 64-tile block per workgroup

__global__ __launch_bounds__(kTileFlagThreads) void tile_flags_kernel(const float* __restrict__ g_rgb,
                                                                      const float* __restrict__ g_sigma, int64_t M,
                                                                      int dense,
                                                                      uint8_t* __restrict__ flags,
                                                                      uint32_t* __restrict__ blk_count) {
    __shared__ uint32_t wcnt[kTileFlagThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t tw = static_cast<int64_t>(blockIdx.x) * 64 + wv * 16;
    bool nz[8];
    // lanes 0-31: tile tw + 2 it, lanes 32-63: tile tw + 2 it + 1 (one sample each)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int64_t m = (tw + 2 * it + (lane >> 5)) * 32 + (lane & 31);
        bool v = false;
        if (m < M) {
            if (dense) {
                v = true;
            } else {
                const float r0 = g_rgb[3 * m], r1 = g_rgb[3 * m + 1], r2 = g_rgb[3 * m + 2], s0 = g_sigma[m];
                v = (r0 != 0.f) | (r1 != 0.f) | (r2 != 0.f) | (s0 != 0.f);  // NaN counts as nonzero
            }
        }
        nz[it] = v;
    }
    uint32_t mask = 0;  // bit k: tile tw + k is active (wave-uniform); tiles past the last sample: 0
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const uint64_t b = __ballot(nz[it]);
        mask |= (static_cast<uint32_t>(b & 0xffffffffull) != 0 ? 1u : 0u) << (2 * it);
        mask |= (static_cast<uint32_t>(b >> 32) != 0 ? 1u : 0u) << (2 * it + 1);
    }
    if (lane < 16) flags[tw + lane] = static_cast<uint8_t>((mask >> lane) & 1u);
    if (lane == 0) wcnt[wv] = __popc(mask);
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
}

// ------------------------------------------------------------------ dW ----
// Workgroup = (job, chunk of tiles): 8 waves, each accumulating its planned share
// (DwWave: up to 5x2 blocks) of the job's NBz x KB output grid.  Per tile the
// job's dz and input blocks (every tensor once: h_{n-1} feeds the feature layer
// and the sigma head in one job) are staged into LDS by LDS-DMA (a 4-stage ring of
// 1-KB wave pieces) and the sample-major MFMA operands are rebuilt from the
// B-operand images.  Bias partials are v_dot2 sums of the dz operands.  Output
// slab per chunk: [dz row][input col | bias] fp32.  The kernel runs at its staging
// ceiling: the same staging with the MFMAs compiled out (a timing-only variant,
// r02) is within 1 % of it.
#ifndef NR_DW_AUX
#define NR_DW_AUX 0  // cache-policy bits of the dW staging loads (2: nt)
#endif

// Block-local feature of dW operand row/col index r: r = 16h + i <-> accumulator
// register i of lane half h in the B-operand image.
__device__ __forceinline__ int dw_feat(int r) { return acc_row(r & 15, r >> 4); }

// bf16 staging swizzle: image lane L of fragment s sits in LDS slot
// L ^ 4*(L>>5 & 1) ^ 8*s (an involution), which makes the transpose reads of
// dw_frag_bf16 bank-conflict free (the 16 slots a 32-lane half reads are
// distinct mod 16).  glds writes lane-linear, so the swizzle goes on the source.
__device__ __forceinline__ int dw_slot(int L, int s) { return L ^ (((L >> 5) & 1) << 2) ^ (s << 3); }
// fp32 staging: fragment f's 16-B chunk c lands at chunk position c ^ 2 (f + 4 (c >> 5))
// (an involution: bits 1-3 only), so the per-sample reads of mlp_dw_kernel's fp32 path
// spread over all 16 four-bank groups instead of 2 (8-way conflicts)
__device__ __forceinline__ int dw_slot32(int L, int f) { return L ^ (2 * (f + 4 * ((L >> 5) & 1))); }

// ds_read_b64_tr_b16 through inline asm: the builtin makes hipcc wait vmcnt(0)
// (every in-flight LDS-DMA stage) before each read, which would serialise the
// staging pipeline.  The caller waits lgkmcnt itself (tr_wait) before use.
template <int OFF>
__device__ __forceinline__ void tr16(uint64_t& out, uint32_t addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(out) : "v"(addr), "i"(OFF));
}

// the two 64-bit halves of a transpose-read operand as one bf16x8 (a pure bit cast, so
// the register allocator can place the two asm outputs as the halves: no copies)
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
// ds_read_b32 through inline asm (as tr16: no compiler drain of in-flight LDS-DMA)
template <int OFF>
__device__ __forceinline__ void ds_rd32(float& out, uint32_t addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(out) : "v"(addr), "i"(OFF));
}

__device__ __forceinline__ bf16x8 tr_pair(uint64_t lo, uint64_t hi) {
    return __builtin_bit_cast(bf16x8, u64x2_t{lo, hi});
}

// LDS byte offsets, within a staged block, of the two transpose reads that give
// lane l its bf16 operand for k-step ks: lane l = 16g + i (h = g&1, hh = g>>1)
// receives feature acc_row(i, h) of samples 16ks + 8hh + 0..7 (two reads of 4
// samples x 16 features; lane 4q+p of a group addresses sample q, features
// 4p..4p+3: cdna_hip_programming.md T10).
__device__ __forceinline__ uint32_t dw_tr_off(int ks, int half, int lane) {
    const int g = lane >> 4, h = g & 1, hh = g >> 1;
    const int lam = lane & 15, q = lam >> 2, p = lam & 3;
    const int s = p >> 1;
    const int L = 16 * ks + 8 * hh + q + 32 * h + 4 * half;
    return static_cast<uint32_t>(s * kFragBytes + dw_slot(L, s) * 16 + 8 * (p & 1));
}

// acc + the four 16-bit values of a transpose read (bias partial sums): two
// v_dot2c_f32_{bf16,f16} against (1, 1), fp32 accumulation
template <int PREC>
__device__ __forceinline__ float dw_acc4(uint64_t v, float acc) {
    const unsigned w0 = static_cast<unsigned>(v), w1 = static_cast<unsigned>(v >> 32);
    if constexpr (PREC == NR_PREC_FP16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 one = __builtin_bit_cast(h2, 0x3c003c00u);
        acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w0), one, acc, false);
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, w1), one, acc, false);
    } else {
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        const b2 one = __builtin_bit_cast(b2, 0x3f803f80u);
        acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2, w0), one, acc, false);
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2, w1), one, acc, false);
    }
}

template <int PREC>
__global__ __launch_bounds__(kDwThreads, 1) void mlp_dw_kernel(DwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar staging loop
    // chunk-major (wg_map): every job of a chunk runs at about the same time (an input two
    // jobs share, x_enc of the x-jobs beyond the first, is re-read from L2/MALL)
    const int wmap = a.wg_map[blockIdx.x];
    const int j = wmap & 31, chunk = wmap >> 5;
    const int NBz = a.job_NBz[j], KB = a.job_KB[j];
    const int winfo = a.job_wave[j][wv];
    const int row0 = winfo & 63, np = (winfo >> 6) & 7, col0 = (winfo >> 9) & 63, nq = (winfo >> 15) & 3;
    const bool active = np > 0;
    const bool do_bias = active && ((winfo >> 17) & 1);
    // this chunk's entries [t0, t1) of the active-tile list: ceil(count / chunks) each, in
    // list order (with every tile active, exactly the dense form's contiguous ranges)
    const int64_t cnt = *a.count;
    const int64_t tpc = (cnt + a.job_chunks[j] - 1) / a.job_chunks[j];
    const int64_t t0 = static_cast<int64_t>(chunk) * tpc;
    int64_t t1 = t0 + tpc;
    if (t1 > cnt) t1 = cnt;
    constexpr int FPB = kFPB<PREC>;
    constexpr int BLK = FPB * kFragBytes;

    // Stage tile t into buffer b (the job's blocks, dz segments first).  Every wave
    // issues exactly `per_wave` 1-KB LDS-DMA pieces per tile (padding pieces re-load
    // piece 0 into a scratch KB), so a counted vmcnt can retire one stage while the
    // next NS-2 stay in flight across the barrier.  Each piece's per-lane source
    // address, per-tile stride and LDS offset are resolved once per workgroup: the
    // per-tile staging is one pointer bump and one DMA per piece (the segment walk
    // per piece and tile made this kernel SALU-bound).
    const int total = (NBz + KB) * FPB;
    const int per_wave = (total + kDwWaves - 1) / kDwWaves;
    constexpr int kMaxPW = dw_max_pieces(k16<PREC>);  // the plan keeps per_wave <= kMaxPW
    const char* psrc[kMaxPW];  // piece k of tile 0 (lane's 16 B); tile t adds t * pstride[k]
    int64_t pstride[kMaxPW];
    int pdst[kMaxPW];  // LDS offset within a stage, or -1: scratch KB
#pragma unroll
    for (int k = 0; k < kMaxPW; ++k) {
        psrc[k] = nullptr;
        pstride[k] = 0;
        pdst[k] = -1;
        if (k < per_wave) {
            int pc = wv + k * kDwWaves;
            const bool pad = pc >= total;
            if (pad) pc = 0;
            int sg = 0, p0 = 0;
            while (pc >= p0 + a.seg_blocks[j][sg] * FPB) p0 += a.seg_blocks[j][sg++] * FPB;
            const int nb = a.seg_blocks[j][sg];
            const int L = k16<PREC> ? dw_slot(lane, (pc - p0) % FPB) : dw_slot32(lane, (pc - p0) % FPB);
            pstride[k] = static_cast<int64_t>(nb) * BLK;
            psrc[k] = a.seg_ptr[j][sg] + (pc - p0) * kFragBytes + L * 16;
            pdst[k] = pad ? -1 : pc * kFragBytes;
        }
    }
    // this chunk's list entries, copied into LDS once when they fit (a scalar load per
    // stage would wait on the L2 inside the tile loop: lgkmcnt also counts the transpose reads)
    const uint32_t* lds_list = nullptr;
    if (a.list_lds && cnt != a.tiles) {  // (every tile active: the list is the identity)
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds + a.list_lds);
        for (int64_t q = t0 + tid; q < t1; q += kDwThreads) dst[q - t0] = a.list[q];
        __syncthreads();  // (before any staging DMA is in flight)
        lds_list = dst;
    }
    // the tile of list entry pos: with every tile active the list is the identity (no read:
    // the dense form's cost); else from the LDS copy through asm with its own wait (a
    // compiler-visible LDS load behind the staging DMA makes hipcc wait vmcnt(0) for the
    // DMA, which writes LDS), or from the global list when the copy did not fit
    const bool ident = cnt == a.tiles;
    const uint32_t list_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_list));
    auto tile_at = [&](int64_t pos) -> int64_t {
        if (ident) return pos;
        if (!lds_list) return a.list[pos];
        uint32_t v;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)"
                     : "=v"(v)
                     : "v"(list_base + 4u * static_cast<uint32_t>(pos - t0))
                     : "memory");
        return __builtin_amdgcn_readfirstlane(v);
    };
    // stage `tile` into buffer b
    auto stage = [&](int b, int64_t tile) {
        char* dst = lds + b * a.stage_bytes;
        char* scratch = lds + a.nstage * a.stage_bytes;
#pragma unroll
        for (int k = 0; k < kMaxPW; ++k) {
            if (k < per_wave) {
                char* d = pdst[k] < 0 ? scratch : dst + pdst[k];
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(psrc[k] + tile * pstride[k]),
                    (__attribute__((address_space(3))) void*)(d), 16, 0, NR_DW_AUX);
            }
        }
    };
    // wait until at most n of this wave's pieces are outstanding (n: wave-uniform)
    auto wait_pieces = [](int n) {
        switch (n) {
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
    };

    uint32_t trof[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) trof[ks][hf] = dw_tr_off(ks, hf, lane);
    const int NS = a.nstage;
    float* slab = a.slabs + static_cast<int64_t>(chunk) * a.slab_floats_per_chunk + a.job_slab[j];
    const int ld = KB * 32 + 1;
    const int hl = lane >> 5, ml = lane & 31;

    // The tile loop and the slab write for a compile-time share shape NP x NQ (16-bit:
    // the share's np x nq blocks run as the next compiled shape up, the extra blocks
    // accumulate garbage that is never written; fp32: kDwMaxP x kDwMaxQ with runtime
    // validity).  Each shape's accumulators live only inside its own instantiation.
    using std::integral_constant;
    auto run = [&](auto npc, auto nqc) {
        constexpr int NP = decltype(npc)::value, NQ = decltype(nqc)::value;
        f32x16 acc[NP][NQ];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int q = 0; q < NQ; ++q) zero(acc[p][q]);
        float bsum[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) bsum[p] = 0.f;
        bool nval[NP], kval[NQ];
#pragma unroll
        for (int p = 0; p < NP; ++p) nval[p] = p < np;
#pragma unroll
        for (int q = 0; q < NQ; ++q) kval[q] = q < nq;

        for (int k = 0; k < NS - 1; ++k)
            if (t0 + k < t1) stage(k, tile_at(t0 + k));
        int bcur = 0, bnext = NS - 1;  // stage of tile t, stage tile t+NS-1 goes to
        for (int64_t t = t0; t < t1; ++t) {
            // stages t+1 .. t+NS-2 may stay in flight
            int64_t ahead = t1 - 1 - t;
            if (ahead > NS - 2) ahead = NS - 2;
            wait_pieces(per_wave * static_cast<int>(ahead));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (t + NS - 1 < t1) stage(bnext, tile_at(t + NS - 1));
            bnext = bnext + 1 == NS ? 0 : bnext + 1;
            const char* buf = lds + bcur * a.stage_bytes;
            bcur = bcur + 1 == NS ? 0 : bcur + 1;
            if (!active) continue;
            if constexpr (k16<PREC>) {
                const uint32_t base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(buf));
                const uint32_t bufA = base + row0 * BLK, bufB = base + (NBz + col0) * BLK;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    uint64_t ra[NP][2], rb[NQ][2];
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const uint32_t oa = bufA + trof[ks][hf], ob = bufB + trof[ks][hf];
                        rbm_static_for<NP>(
                            [&](auto pp) { tr16<decltype(pp)::value * BLK>(ra[decltype(pp)::value][hf], oa); });
                        rbm_static_for<NQ>(
                            [&](auto qq) { tr16<decltype(qq)::value * BLK>(rb[decltype(qq)::value][hf], ob); });
                    }
                    // the wait publishes the transpose reads: tie every destination to it
                    // (volatile asm keeps its order) so no use is scheduled above it
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
                        for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(ra[p][hf]));
#pragma unroll
                        for (int q = 0; q < NQ; ++q) asm volatile("" : "+v"(rb[q][hf]));
                    }
                    bf16x8 A[NP], Bm[NQ];
#pragma unroll
                    for (int p = 0; p < NP; ++p) A[p] = tr_pair(ra[p][0], ra[p][1]);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) Bm[q] = tr_pair(rb[q][0], rb[q][1]);
                    // branch-free: per-MFMA validity branches made this loop SALU-bound
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[p][q] = mfma16<PREC>(A[p], Bm[q], acc[p][q]);
                    // bias gradient = dz summed over samples: lane-local fp32 partials
                    if (do_bias)
#pragma unroll
                        for (int p = 0; p < NP; ++p) bsum[p] = dw_acc4<PREC>(ra[p][1], dw_acc4<PREC>(ra[p][0], bsum[p]));
                }
            } else {
                // fp32 image [tq][L][4]: operand row r <-> (hh = r>>4, reg i = r&15 -> frag i>>2,
                // elem i&3); sample m = 2 ss + kk is 16-B chunk 32 hh + m of the fragment,
                // staged at chunk position 32 hh + 2 (ss ^ k2) + kk (dw_slot32, k2 = frag + 4 hh):
                // the 16 chunks one read instruction touches fall in 16 distinct 4-bank groups
                const int r = lane & 31, kk = lane >> 5;
                const int hh = r >> 4, i = r & 15;
                const int k2 = (i >> 2) + 4 * hh;
                const uint32_t base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(buf)) +
                                      ((i >> 2) * 64 + 32 * hh + kk) * 16 + (i & 3) * 4;
                const uint32_t bufA = base + row0 * BLK, bufB = base + (NBz + col0) * BLK;
                const uint32_t kx = static_cast<uint32_t>(k2) << 5;
                // operands through asm reads (a plain LDS load makes the compiler drain every
                // in-flight staging DMA first), one sample pair read ahead; the compiled
                // share shape runs branch-free (blocks past np x nq accumulate garbage that
                // is never written, as in the 16-bit path)
                float Ar[2][NP], Br[2][NQ];
                auto rd = [&](auto sc) {
                    constexpr int ss = decltype(sc)::value;
                    // (ss ^ k2) << 5 computed in place: sixteen hoisted per-lane offsets would
                    // cost sixteen registers across the tile loop
                    uint32_t o;
                    asm volatile("v_xor_b32 %0, %1, %2" : "=v"(o) : "i"(ss << 5), "v"(kx));
                    const uint32_t oa = bufA + o, ob = bufB + o;
                    rbm_static_for<NP>([&](auto pp) { ds_rd32<decltype(pp)::value * BLK>(Ar[ss & 1][decltype(pp)::value], oa); });
                    rbm_static_for<NQ>([&](auto qq) { ds_rd32<decltype(qq)::value * BLK>(Br[ss & 1][decltype(qq)::value], ob); });
                };
                rd(integral_constant<int, 0>{});
                rbm_static_for<16>([&](auto sc) {
                    constexpr int ss = decltype(sc)::value;
                    if constexpr (ss + 1 < 16) {
                        rd(integral_constant<int, ss + 1>{});
                        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NP + NQ) : "memory");
                    } else {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(Ar[ss & 1][p]));
#pragma unroll
                    for (int q = 0; q < NQ; ++q) asm volatile("" : "+v"(Br[ss & 1][q]));
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        bsum[p] += Ar[ss & 1][p];  // summed by every wave, written by the bias share's
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[p][q] = mfma_f32(Ar[ss & 1][p], Br[ss & 1][q], acc[p][q]);
                    }
                });
            }
        }
        if (!active) return;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (!nval[p]) continue;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (!kval[q]) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * (row0 + p) + dw_feat(acc_row(r, hl));
                    const int col = 32 * (col0 + q) + dw_feat(ml);
                    slab[static_cast<int64_t>(row) * ld + col] = acc[p][q][r];
                }
            }
            if (do_bias) {
                // lanes l and l+32 summed the two sample halves of operand row l & 31
                const float tot = bsum[p] + __shfl_xor(bsum[p], 32);
                if (hl == 0) slab[static_cast<int64_t>(32 * (row0 + p) + dw_feat(ml)) * ld + KB * 32] = tot;
            }
        }
    };
    if constexpr (!k16<PREC>) {
        // fp32: the plan keeps every share within 4 x 2 (the sigma head is its own job), so
        // one compiled 4x2 share: a wave pair on one SIMD runs 16 blocks per tile of an
        // h-job instead of the 20 of the 5x2 shape (a second shape in the kernel spills)
        run(integral_constant<int, 4>{}, integral_constant<int, kDwMaxQ>{});
    } else {
        // compiled shares: 1x2, 4x1, 4x2, 5x2 (a smaller share runs the next one up)
        if (np <= 1)
            run(integral_constant<int, 1>{}, integral_constant<int, 2>{});
        else if (np <= 4 && nq <= 1)
            run(integral_constant<int, 4>{}, integral_constant<int, 1>{});
        else if (np <= 4)
            run(integral_constant<int, 4>{}, integral_constant<int, 2>{});
        else
            run(integral_constant<int, kDwMaxP>{}, integral_constant<int, kDwMaxQ>{});
    }
}

// One workgroup per (reduce range k = blockIdx.y, output row r = blockIdx.x): the row's
// weight columns and its bias (column `in`) across the threads, so neither an index
// search per parameter nor a division; consecutive columns read consecutive slab floats.
__global__ void mlp_dw_reduce_kernel(ReduceArgs a) {
    const int k = blockIdx.y, r = blockIdx.x;
    if (r >= a.rows[k]) return;
    const int in = a.in[k];
    const int64_t st = a.slab_floats_per_chunk;
    for (int c = threadIdx.x; c <= in; c += blockDim.x) {
        int job = -1, row = 0, col = 0;
        int64_t dst;
        if (c < in) {
            for (int q = 0; q < a.nseg[k]; ++q) {
                const RedSeg& sg = a.seg[k][q];
                if (c >= sg.col0 && c < sg.col0 + sg.width) {
                    job = sg.job;
                    row = sg.slab_row0 + r;
                    col = sg.slab_col0 + (c - sg.col0);
                }
            }
            dst = a.w_off[k] + static_cast<int64_t>(r) * in + c;
        } else {
            job = a.bjob[k];
            row = a.brow0[k] + r;
            col = a.job_KB[job] * 32;
            dst = a.b_off[k] + r;
        }
        if (job < 0) continue;
        const int ld = a.job_KB[job] * 32 + 1;
        const float* s = a.slabs + a.job_slab[job] + static_cast<int64_t>(row) * ld + col;
        // chunk order fixed (deterministic); loads issued four at a time
        const int nch = a.job_chunks[job];
        float acc = 0.f;
        int ch = 0;
        for (; ch + 4 <= nch; ch += 4) {
            const float v0 = s[ch * st], v1 = s[(ch + 1) * st], v2 = s[(ch + 2) * st], v3 = s[(ch + 3) * st];
            acc = (((acc + v0) + v1) + v2) + v3;
        }
        for (; ch < nch; ++ch) acc += s[ch * st];
        a.g[dst] = acc * a.inv_gscale;
    }
}

int launch_tile_flags(const float* g_rgb, const float* g_sigma, int64_t M, int dense, int64_t nseg, uint8_t* flags,
                      uint32_t* blk_count, hipStream_t s) {
    hipLaunchKernelGGL(tile_flags_kernel, dim3(static_cast<unsigned>(nseg * (kSegTiles / 64))), dim3(kTileFlagThreads),
                       0, s, g_rgb, g_sigma, M, dense, flags, blk_count);
    return check_launch("nr_mlp_backward_dx (tile flags)");
}

int launch_dw(int prec, const DwArgs& a, int nwg, size_t lds, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(nwg)), block(kDwThreads);
    if (prec == NR_PREC_BF16)
        hipLaunchKernelGGL(mlp_dw_kernel<NR_PREC_BF16>, grid, block, lds, s, a);
    else if (prec == NR_PREC_FP16)
        hipLaunchKernelGGL(mlp_dw_kernel<NR_PREC_FP16>, grid, block, lds, s, a);
    else
        hipLaunchKernelGGL(mlp_dw_kernel<NR_PREC_FP32>, grid, block, lds, s, a);
    return check_launch("nr_mlp_backward_dw");
}

int launch_dw_reduce(const ReduceArgs& a, int max_rows, hipStream_t s) {
    hipLaunchKernelGGL(mlp_dw_reduce_kernel, dim3(static_cast<unsigned>(max_rows), static_cast<unsigned>(a.n_red)),
                       dim3(256), 0, s, a);
    return check_launch("nr_mlp_backward_reduce");
}

}  // namespace nr

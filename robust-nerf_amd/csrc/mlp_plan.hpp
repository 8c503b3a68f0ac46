// Layout plan of the fused NeRF MLP (reference noisy_src/model.py:83-221).
//
// Everything the host entry points and the kernels agree on lives here:
//   * the flat fp32 parameter layout (nn.Module.parameters() order),
//   * the packed MFMA fragment images of W (forward) and W^T (backward),
//     stored chunk-major: one chunk = every row block of one 32-wide k block,
//     i.e. exactly what the kernels stream through LDS per step, each
//     direction's images laid out in its stream order;
//   * fp32 vectors (biases, w_sigma, W_rgb) in accumulator-register order;
//   * the activations saved by a training forward and the per-layer
//     pre-activation gradients dz written by the backward, both stored as
//     MFMA B-operand images: per 32-sample tile and 32-feature block, FPB
//     wave-wide 1-KB fragments (lane L = sample + 32*h holds 16 B), so every
//     store is a fully coalesced 1-KB wave write.
// ReLU masks are bitmasks in accumulator-register order (16 B per lane per layer).
#pragma once

#include <cstddef>
#include <cstdint>

#include "nerf_hip.h"

namespace nr {

constexpr int kHidden = 256;           // ModelConfig.hidden_dim supported by the kernels
constexpr int kHB = kHidden / 32;      // hidden feature blocks
constexpr int kMaxTrunk = 16;          // num_hidden_layers upper bound
constexpr int kMaxMfmaLayers = kMaxTrunk + 2;  // trunk + feature + dir
constexpr int kFragBytes = 1024;       // one wave-wide 16-B-per-lane operand fragment
constexpr int kScratchTiles = 64;  // dX waves without an active tile spread their stores over these
constexpr int kSegTiles = 256;  // tiles per segment of the active-tile list
constexpr int kMaxJobs = kMaxTrunk + 8;  // dW jobs: x-jobs + trunk h-jobs + feat + heads + dir
constexpr int kMaxSeg = 2;
constexpr int kMaxJobSeg = 4;            // tensors on either side of a dW job
constexpr int kMaxRed = kMaxTrunk + 4;    // reduce ranges: trunk, feat, sigma, rgb, dir
// fp32 weight streams (StreamDesc below): chunks per stream, >= the sum of KB (forward) or
// NB (backward) over the MFMA layers of every config make_plan accepts: the stream builders
// refuse a stream that does not fit, so make_plan refuses its config
constexpr int kMaxChunks = 176;
// dW workgroups: 8 waves, each issuing at most dw_max_pieces 1-KB LDS-DMA pieces per tile
constexpr int kDwThreads = 512;
constexpr int kDwWaves = kDwThreads / 64;
__host__ __device__ constexpr int dw_max_pieces(bool k16) { return k16 ? 6 : 10; }
constexpr int kDwMaxWgs = 256;          // one round of workgroups (make_sizes: NR_DW_WGS)
constexpr int kDwLdsBytes = 160 * 1024;  // a workgroup's LDS: the staging ring, 1 KB of scratch, the chunk's list
#ifndef NR_DW_NSTAGE
#define NR_DW_NSTAGE 4  // LDS staging ring depth of the dW kernel (tiles)
#endif
// The 1-KB pieces a dW job may stage per tile, (NBz + KB) * FPB of them: what its waves can
// issue, and a stage must fit twice in LDS beside the scratch (the ring needs two)
constexpr int dw_max_stage_pieces(bool k16) {
    constexpr int twice = (kDwLdsBytes - kFragBytes) / (2 * kFragBytes);
    return kDwWaves * dw_max_pieces(k16) < twice ? kDwWaves * dw_max_pieces(k16) : twice;
}

// One input segment of a linear layer: columns [col0, col0+width) of W,
// occupying ceil(width/32) consecutive 32-wide input blocks.
struct Seg {
    int col0, width, blocks;
};

struct LinearDesc {
    int64_t w_off, b_off;  // offsets into the flat parameter buffer (floats)
    int out, in;           // nn.Linear shape (out, in)
    int NB, KB;            // output / input 32-blocks (padded)
    int nseg;
    Seg seg[kMaxSeg];
    int64_t pk_fwd, pk_bwd;  // byte offsets of the W / W^T fragment images
    int64_t pk_bwdr;         // 16-bit: row-block-major W^T image of the h (feat) input rows (dX chain)
    int64_t vb;              // byte offset of the bias vector image (accumulator order)
};

// A tensor range of a dW job: `blocks` consecutive 32-feature blocks of
// saved (is_ws = 0) or workspace (is_ws = 1) tensor `tensor`.
struct DwSeg {
    int is_ws, tensor, blocks;
};

// One wave's share of a dW job: dz row blocks [row0, row0+np) x input column
// blocks [col0, col0+nq) (np <= kDwMaxP, nq <= kDwMaxQ), plus the bias partial
// sums of those dz rows when bias != 0.
constexpr int kDwMaxWaves = kDwWaves;
constexpr int kDwMaxP = 5, kDwMaxQ = 2;
struct DwWave {
    int row0, np, col0, nq, bias;
};

// A dW job: products dz^T . in over the tiles of one chunk, for the 32x32 blocks
// its waves list, inside an NBz x KB grid (dz segments stacked as rows, input
// segments as columns; every tensor is staged once per tile).  Output slab per
// chunk: (NBz*32) x (KB*32 + 1) floats, the last column holding the bias partial
// sums of the dz rows; blocks no wave lists are never written or read.
struct DwJob {
    int ndz, nin;
    DwSeg dz[kMaxJobSeg], in[kMaxJobSeg];
    int NBz, KB;
    int64_t slab_off;  // float offset of this job's slab inside one chunk's slab set
    int nwaves;
    DwWave w[kDwMaxWaves];
};

// Saved tensor ids (training forward) and workspace tensor ids (backward).
enum SavedId { SV_XENC = 0, SV_H0 = 1 /* .. SV_H0+n_layers-1 */ };
enum WsId { WS_DZ0 = 0 /* dz of trunk i: WS_DZ0+i; then feat, dir, heads */ };

// Per-parameter-range map for the slab reduction: W (rows x in, at w_off) takes
// its column segments from job slabs (slab row slab_row0 + r, column
// slab_col0 + c - col0); the bias (b_off, rows) from job bjob's bias column.
struct RedSeg {
    int col0, width, job, slab_row0, slab_col0;
};
struct ReduceRange {
    int rows, in;
    int64_t w_off, b_off;
    int nseg;
    RedSeg seg[kMaxSeg];
    int bjob, brow0;
};

struct MlpPlan {
    int L, Ld, n_layers, use_vd, prec;
    int dense_bwd;                    // NrMlpConfig.dense_backward: every tile through the backward
    uint32_t skips;
    int pos_dim, dir_dim, XB, DB;
    int64_t param_count;
    int n_lin;                        // trunk + feat + dir (MFMA layers)
    LinearDesc lin[kMaxMfmaLayers];   // [0, n_layers) trunk, n_layers feat, n_layers+1 dir
    int64_t sig_w, sig_b, rgb_w, rgb_b;
    int64_t packed_bytes;
    int64_t vsig, vrgb;               // byte offsets of the w_sigma / W_rgb vector images
    int64_t vhead;                    // 16-bit forward: w_sigma then the 3 W_rgb rows as vector images (3 KB)
    int esize;                        // bytes per saved/workspace element (2 bf16, 4 fp32)
    int fpb;                          // 1-KB fragments per 32x32 block (2 bf16, 4 fp32)
    // saved tensors
    int n_saved;                      // xenc, h0..h_{n-1}, feat, denc, hc
    int sv_feat, sv_denc, sv_hc;
    int sv_F[kMaxTrunk + 4];          // padded features per saved tensor
    int n_mask;                       // mask words: trunk layers + hc
    // workspace tensors
    int n_ws;                         // dz_0..dz_{n-1}, dz_feat, dz_dir, dz_heads
    int ws_feat, ws_dir, ws_heads;
    int ws_F[kMaxTrunk + 3];
    // dW jobs and the reduction map
    int n_jobs;
    DwJob job[kMaxJobs];
    int dw_stage_bytes, dw_nstage;    // the dW staging ring: the largest job's blocks of one tile, 2..NR_DW_NSTAGE times
    int64_t slab_floats_per_chunk;
    int n_red;
    ReduceRange red[kMaxRed];
};

inline bool is_skip(const MlpPlan& p, int i) { return (p.skips >> i) & 1u; }

// fp16 backward runs on dz scaled by 2^14 (the per-sample gradients of a mean
// loss over 4096 rays sit near 1e-6, in fp16's subnormal range); the dW reduce and
// the input gradients divide it out exactly.
inline float grad_scale(int prec) { return prec == NR_PREC_FP16 ? 16384.0f : 1.0f; }

// Builds the plan; returns false (with *why set) for unsupported configs: everything about a
// launch that the config alone decides is checked here (the fp32 weight streams, the dW
// shares and staging), so a config that gets a plan has a launch at every M but those the
// entry points refuse by M.
bool make_plan(const NrMlpConfig* cfg, MlpPlan* p, const char** why);

// Byte sizes / offsets that depend on the number of samples.
struct MlpSizes {
    int64_t tiles;
    int64_t tiles_alloc;  // tiles rounded up to whole 16-tile groups (every fwd wave may store its tile),
                          // then kScratchTiles scratch tiles (dX waves without a tile store there)
    int64_t saved_off[kMaxTrunk + 4];  // bytes
    int64_t mask_off;                  // bytes
    int64_t saved_bytes;
    int64_t ws_off[kMaxTrunk + 3];     // bytes
    int chunks;                        // dW split over sample tiles
    int job_chunks[kMaxJobs];          // dW workgroups of each job (16-bit: all = chunks; fp32: by cost)
    int max_chunks;                    // per-chunk slab sets allocated (the largest job_chunks)
    int64_t slab_off;                  // bytes
    int64_t nseg;                      // segments of kSegTiles tiles
    // bytes: tile flags (u8, nseg * kSegTiles); 64-tile block counts; the dW list; its length
    int64_t flags_off, blkcnt_off, dwlist_off, count_off;
    int64_t ws_bytes;
};

MlpSizes make_sizes(const MlpPlan& p, int64_t M);

// Frozen field (nr_mlp_forward_frozen / nr_mlp_backward_input): what a backward that
// produces g_x / g_d alone reads, and nothing else.
//
// 16-bit.  saved_frozen is the ReLU mask region by itself: tiles * n_mask KB, tile-major
// ([tile][mask word][64 lanes x 16 B], as the training layout's mask region, at offset
// 0), with no padding tiles: forward waves past the last tile store nothing, and dX waves
// without a tile read tile 0's masks (their inputs are zero).  The workspace, in order,
// every part 256-byte aligned:
//   dz image of each x_enc-reading trunk layer (layer 0 and every layer after a skip), in
//     layer order: (tiles + kScratchTiles) tiles x kHB blocks x 2 KB
//   dz_c image: (tiles + kScratchTiles) tiles x kHB/2 blocks x 2 KB
//   tile flags: nseg * kSegTiles bytes
//   64-tile block counts: nseg * (kSegTiles / 64) uint32
// The scratch tiles (dX waves without an active tile store there) are tiles
// [tiles, tiles + kScratchTiles) of every image.  No dz_heads, dz_feat or other trunk
// dz, no dW list, count or slabs.
//
// fp32 (parity mode): the chunk-major backward reads the saved activations, so both
// buffers have the training layout and sizes (make_sizes).
struct FrozenSizes {
    int64_t tiles, nseg;
    int64_t saved_bytes;               // mask_off is 0
    uint32_t keep_dz;                  // bit l: trunk layer l's dz image is in the workspace
    int64_t dz_off[kMaxTrunk];         // bytes, valid for the layers of keep_dz
    int64_t dz_dir_off, flags_off, blkcnt_off;
    int64_t scratch_base;              // first scratch tile of the images
    int64_t ws_bytes;
};

FrozenSizes make_frozen_sizes(const MlpPlan& p, int64_t M);

// What the 16-bit input-gradient pass (mlp_dinput_kernel) reads of a workspace, in either
// layout: the tile flags, and the dz images of the x_enc-reading trunk layers (layer 0 and
// every layer after a skip; the other entries of dz_off are 0) and of the dir layer.
struct DinOffsets {
    int64_t tiles;
    int64_t flags_off;
    int64_t dz_off[kMaxTrunk];  // bytes, by trunk layer
    int64_t dz_dir_off;
};

DinOffsets din_offsets(const MlpPlan& p, const MlpSizes& z);
DinOffsets din_offsets(const MlpPlan& p, const FrozenSizes& f);  // 16-bit (fp32 has the training layout)

// ---------------------------------------------------------- launch descriptors ----
// What the fp32 chains, the dW GEMM and its reduction take of the plan, each built by one
// pure function of (plan, sizes, base pointers) that the entry points (mlp.hip) launch with
// and the host checker (tests/native/plan_check.cpp) inspects.  The structs are kernel
// arguments: their layout is the kernels'.

// An fp32 weight stream: a sequence of chunks (all row blocks of one k block of one layer
// image) consumed in order through two LDS slots of the largest chunk's size.
struct StreamDesc {
    int64_t base;                  // byte offset of the stream's first chunk in `packed`
    int nq;                        // chunks
    int ckb[kMaxChunks];           // bytes loaded per chunk, in KB
    int cadv[kMaxChunks];          // bytes to the next chunk, in KB (>= ckb: a chunk may be loaded in part)
};
// the forward's largest chunk is 8 row blocks of a layer's W; the backward's the skip
// layer's W^T, (XB + 8) row blocks
constexpr int kFwdSlotMax = 32 * 1024, kBwdSlotMax = 40 * 1024;

// The forward stream (W images: trunk 0..n-1, feat, dir) and the backward stream (W^T
// images: dir, feat, trunk n-1..1, and trunk 0 when want_x), with *slot_bytes the size of an
// LDS slot.  Without want_x a skip layer's and the dir layer's chunks are loaded in part:
// [h rows | x_enc rows] and [feat rows | d_enc rows], of which only the first 8 row blocks
// feed anything but g_x / g_d.  false (with *why) for a stream of more than kMaxChunks chunks
// or a slot beyond kFwdSlotMax / kBwdSlotMax.  make_plan calls them with a null sd, which
// checks the same without writing a table, and refuses an fp32 config they refuse.
bool fwd_stream(const MlpPlan& p, StreamDesc* sd, int* slot_bytes, const char** why);
bool bwd_stream(const MlpPlan& p, bool want_x, StreamDesc* sd, int* slot_bytes, const char** why);

struct DwArgs {
    float* slabs;
    int njobs;
    int64_t tiles;
    const uint32_t* list;           // active tiles in order and their count (built during the dX launch)
    const uint32_t* count;
    int list_lds;                   // LDS byte offset the chunk's list entries are staged to (0: read them global)
    int job_chunks[kMaxJobs];       // chunks of each job: list entries split evenly in order
    uint16_t wg_map[kDwMaxWgs];     // workgroup -> job | chunk << 5 (chunk-major: one chunk of every job in a row)
    int stage_bytes, nstage;
    int64_t slab_floats_per_chunk;
    int job_NBz[kMaxJobs], job_KB[kMaxJobs];
    int64_t job_slab[kMaxJobs];
    const char* seg_ptr[kMaxJobs][2 * kMaxJobSeg];  // tensor region: dz segments, then inputs
    uint8_t seg_blocks[kMaxJobs][2 * kMaxJobSeg];
    // wave share (DwWave) packed: row0 | np << 6 | col0 << 9 | nq << 15 | bias << 17; 0 = idle
    int job_wave[kMaxJobs][kDwWaves];
};
static_assert(sizeof(DwArgs) <= 4096, "dW kernel arguments exceed 4 KiB");
static_assert(kMaxJobs <= 32, "wg_map holds the job in 5 bits");

// make_plan keeps row0, col0 and their ends below 64, np <= kDwMaxP and nq <= kDwMaxQ
__host__ __device__ constexpr int dw_wave_pack(int row0, int np, int col0, int nq, int bias) {
    return row0 | np << 6 | col0 << 9 | nq << 15 | bias << 17;
}

// The dW launch over `saved` and `workspace` (16-byte aligned; the list and count are what
// nr_mlp_backward_dx left in the workspace): *w, *nwg workgroups, *lds bytes of dynamic LDS
// (the staging ring, 1 KB of scratch and, when they fit, the largest chunk's list entries).
// false (with *why) when z's chunks make more than kDwMaxWgs workgroups or more LDS than
// kDwLdsBytes; z.max_chunks must be below 2048 (wg_map's 11 bits).
bool dw_args(const MlpPlan& p, const MlpSizes& z, const char* saved, char* workspace, DwArgs* w, int* nwg,
             size_t* lds, const char** why);

// g_params[param] = sum over chunks of its slab entry (fixed chunk order: deterministic).
struct ReduceArgs {
    const float* slabs;
    float* g;
    float inv_gscale;  // fp16: undo the backward's loss scale (a power of two: exact)
    int64_t param_count;
    int64_t slab_floats_per_chunk;
    int n_red;
    int rows[kMaxRed], in[kMaxRed], nseg[kMaxRed], bjob[kMaxRed], brow0[kMaxRed];
    int64_t w_off[kMaxRed], b_off[kMaxRed];
    RedSeg seg[kMaxRed][kMaxSeg];
    int64_t job_slab[kMaxJobs];
    int job_KB[kMaxJobs];
    int job_chunks[kMaxJobs];  // slab sets of each job, summed in chunk order
};

// The reduce launch over the slabs dw_args' launch wrote; returns the longest range's rows
int reduce_args(const MlpPlan& p, const MlpSizes& z, const char* workspace, float* g_params, ReduceArgs* r);

}  // namespace nr

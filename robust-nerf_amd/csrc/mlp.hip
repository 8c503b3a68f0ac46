// Fused NeRF MLP on MFMA (gfx950): the plan and the extern "C" entry points.  An entry point
// is: plan (make_plan refuses a config that has no launch), pointer checks, sizes, the
// launch's arguments, launch.  The weight streams, the dW and the reduce arguments come from
// the pure builders beside the plan (mlp_plan.hpp), the chains' shared blocks from fwd_io /
// dx_io below; the launchers are in the translation units that hold the kernels:
//   mlp_fp32.hip  fp32 parity mode: chunk-major forward and backward dX chain
//   mlp_16.hip    bf16 / fp16: row-block-major forward, dX chain, input gradients
//   mlp_dw.hip    active-tile flags, the dW GEMM and its deterministic split-M reduction
//   mlp_pack.hip  weight packing, the fused optimizer step, the positional-encoding window
//   mlp_dev.hpp   the device helpers they share
//
// Reference: noisy_src/model.py:20-221 — PositionalEncoding (no pi), 8x256 ReLU
// trunk with skip cat([x_enc, h]) after layer 4, sigma = relu(W h), feat = W h
// (no activation), h_c = relu(W [feat, d_enc]), rgb = sigmoid(W h_c).
//
// Formulation.  Every layer computes out^T = W . in^T on 32-sample tiles.  In
// the MFMA C/D layout a lane holds 16 features of ONE sample, so a layer's
// accumulator tile is already the next layer's B operand (packed to bf16 / fp16, or
// as-is in fp32): activations stay in registers through the whole network.
// The A operand (weights) is a packed image whose per-lane 16 bytes per MFMA
// are contiguous, with the k order permuted to match the accumulator rows:
//   16-bit 32x32x16, k-step s: element j <-> input feature 16s + 8(j>>2) + 4h + (j&3)
//   fp32 32x32x2,    k-step t: lane half h <-> input feature (t&3) + 8(t>>2) + 4h
// The images are streamed through an LDS double buffer shared by the workgroup's
// waves, each wave owning one 32-sample tile.
//
// Training saves activations (and the backward its dz) as B-operand images:
// per tile and 32-feature block, FPB wave-wide 1-KB fragments, so each store
// is one coalesced 1-KB wave write.
#include <cmath>
#include <cstring>

#include "mlp_launch.hpp"

#include "mlp_plan.cpp.inc"

using namespace nr;

namespace {

// g[0 .. n) = 0.  A kernel of this library's, not hipMemsetAsync: nr_mlp_backward_dx is
// captured into hipGraphs, and the replayed memset node filled g_x with a stale 16-byte
// pattern instead of zeros (tests/test_tile_patterns.py, the fp32 graph replay)
__global__ void zero_f32_kernel(float* __restrict__ g, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) g[i] = 0.f;
}

bool plan_or_error(const NrMlpConfig* cfg, MlpPlan* p) {
    const char* why = "";
    if (!make_plan(cfg, p, &why)) {
        set_error("NrMlpConfig unsupported: %s", why);
        return false;
    }
    return true;
}

// The forward chains' shared fields (FwdIO's, in RbmArgs or FwdArgs), assigned here and
// nowhere else.  sv_off: the saved tensors' offsets of the training layout (make_sizes), or
// null where none is stored (the frozen field's masks-only forward, whose mask_off is 0)
template <class A>
void fwd_io(A& r, const MlpPlan& p, const void* packed, const float* params, const float* x, const float* d,
            int64_t M, int64_t tiles, float* rgb, float* sigma, void* saved, const int64_t* sv_off, int64_t mask_off) {
    r.packed = static_cast<const char*>(packed);
    r.params = params;
    r.x = x;
    r.d = d;
    r.rgb = rgb;
    r.sigma = sigma;
    r.saved = static_cast<char*>(saved);
    r.M = M;
    r.tiles = tiles;
    r.L = p.L;
    r.Ld = p.Ld;
    r.n_layers = p.n_layers;
    r.skips = p.skips;
    r.sig_b = p.sig_b;
    r.rgb_b = p.rgb_b;
    for (int t = 0; t < p.n_saved; ++t) r.sv_off[t] = sv_off ? sv_off[t] : 0;
    r.sv_feat = p.sv_feat;
    r.sv_denc = p.sv_denc;
    r.sv_hc = p.sv_hc;
    r.mask_off = mask_off;
    r.n_mask = p.n_mask;
}

// The dX chains' shared fields (DxIO's, in BwdrArgs or BwdArgs), assigned here and nowhere
// else.  ws_off: the dz images' offsets by workspace tensor id (p.n_ws of them); dw_list /
// count: null for the input-only chain, which builds no dW list
template <class A>
void dx_io(A& r, const MlpPlan& p, const void* packed, int64_t M, int64_t tiles, int64_t nseg, const float* rgb,
           const float* sigma, const void* saved, int64_t mask_off, const float* g_rgb, const float* g_sigma, char* wsb,
           const int64_t* ws_off, const uint8_t* tflags, const uint32_t* blkcnt, uint32_t* dw_list, uint32_t* count) {
    r.gscale = grad_scale(p.prec);
    r.packed = static_cast<const char*>(packed);
    r.rgb = rgb;
    r.sigma = sigma;
    r.g_rgb = g_rgb;
    r.g_sigma = g_sigma;
    r.saved = static_cast<const char*>(saved);
    r.ws = wsb;
    r.M = M;
    r.tiles = tiles;
    r.flags = tflags;
    r.blk_count = blkcnt;
    r.nseg = nseg;
    r.dw_list = dw_list;
    r.count = count;
    r.n_layers = p.n_layers;
    r.vrgb = p.vrgb;
    r.mask_off = mask_off;
    r.n_mask = p.n_mask;
    for (int t = 0; t < p.n_ws; ++t) r.ws_off[t] = ws_off[t];
    r.ws_feat = p.ws_feat;
    r.ws_dir = p.ws_dir;
    r.ws_heads = p.ws_heads;
}

}  // namespace

extern "C" {

int64_t nr_mlp_param_count(const NrMlpConfig* cfg) {
    MlpPlan p;
    return plan_or_error(cfg, &p) ? p.param_count : -1;
}

int64_t nr_mlp_packed_bytes(const NrMlpConfig* cfg) {
    MlpPlan p;
    return plan_or_error(cfg, &p) ? p.packed_bytes : -1;
}

int64_t nr_mlp_saved_bytes(const NrMlpConfig* cfg, int64_t M) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p) || M < 0) return -1;
    return make_sizes(p, M).saved_bytes;
}

int64_t nr_mlp_workspace_bytes(const NrMlpConfig* cfg, int64_t M) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p) || M < 0) return -1;
    return make_sizes(p, M).ws_bytes;
}

int nr_mlp_pack(const NrMlpConfig* cfg, const float* params, void* packed, nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(params && packed, "nr_mlp_pack: null pointer");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "nr_mlp_pack: packed must be 16-byte aligned");
    return launch_pack(p, params, packed, PackIdx{nullptr, 0}, false, static_cast<hipStream_t>(stream));
}

int nr_mlp_fold_window(const NrMlpConfig* cfg, const float* params, const float* w_pos, const float* w_dir,
                       void* packed, nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(params && packed, "nr_mlp_fold_window: null pointer");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "nr_mlp_fold_window: packed must be 16-byte aligned");
    NR_REQUIRE(!w_dir || p.use_vd, "nr_mlp_fold_window: w_dir without use_view_dirs");
    return launch_fold_window(p, params, packed, w_pos, w_dir, static_cast<hipStream_t>(stream));
}

int nr_mlp_window_grad(const NrMlpConfig* cfg, const float* w_pos, const float* w_dir, float* g_params,
                       nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(g_params, "nr_mlp_window_grad: null pointer");
    NR_REQUIRE(!w_dir || p.use_vd, "nr_mlp_window_grad: w_dir without use_view_dirs");
    if (!w_pos && !w_dir) return NR_OK;  // all ones
    return launch_window_grad(p, w_pos, w_dir, g_params, static_cast<hipStream_t>(stream));
}

int64_t nr_mlp_pack_table_bytes(const NrMlpConfig* cfg) {
    MlpPlan p;
    return plan_or_error(cfg, &p) ? static_cast<int64_t>(kPackSlots) * p.param_count * 4 : -1;
}

int nr_mlp_pack_table(const NrMlpConfig* cfg, uint32_t* table, nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(table, "nr_mlp_pack_table: null pointer");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "nr_mlp_pack_table: table must be 16-byte aligned");
    NR_REQUIRE(p.packed_bytes < kDstMaxOff, "nr_mlp_pack_table: packed images beyond 512 MB");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(table, 0, static_cast<size_t>(kPackSlots) * p.param_count * 4, s);
    if (e != hipSuccess) {
        set_error("nr_mlp_pack_table: %s", hipGetErrorString(e));
        return static_cast<int>(e);
    }
    return launch_pack(p, nullptr, nullptr, PackIdx{table, p.param_count}, true, s);
}

int nr_adam_multi(const NrAdamSpan* spans, int nspan, double lr, double b1, double b2, double eps, int64_t step,
                  const float* sched, nr_stream_t stream) {
    NR_REQUIRE(spans && nspan >= 1 && nspan <= kMaxAdamSpans && step >= 1,
               "nr_adam_multi: bad arguments (1..%d spans, step >= 1)", kMaxAdamSpans);
    AdamMultiArgs a;
    std::memset(&a, 0, sizeof(a));
    int64_t nmax = 0;
    for (int k = 0; k < nspan; ++k) {
        const NrAdamSpan& x = spans[k];
        NR_REQUIRE(x.params && x.grads && x.exp_avg && x.exp_avg_sq && x.n >= 0, "nr_adam_multi: span %d: null buffer", k);
        NR_REQUIRE(((reinterpret_cast<uintptr_t>(x.params) | reinterpret_cast<uintptr_t>(x.grads) |
                     reinterpret_cast<uintptr_t>(x.exp_avg) | reinterpret_cast<uintptr_t>(x.exp_avg_sq) |
                     reinterpret_cast<uintptr_t>(x.pack_table)) & 15) == 0,
                   "nr_adam_multi: span %d: buffers must be 16-byte aligned", k);
        NR_REQUIRE(!x.pack_table || x.packed, "nr_adam_multi: span %d: pack_table without packed", k);
        a.s[k] = AdamSpanDev{x.params, x.grads, x.exp_avg, x.exp_avg_sq, x.n, x.sumsq_partials, x.max_norm,
                             x.pack_table, static_cast<char*>(x.packed)};
        nmax = x.n > nmax ? x.n : nmax;
    }
    if (nmax == 0) return NR_OK;
    // bias corrections in double on the host, as torch's _single/_multi_tensor_adam do
    const double bc1 = 1.0 - std::pow(b1, static_cast<double>(step));
    const double bc2 = 1.0 - std::pow(b2, static_cast<double>(step));
    a.omb1 = static_cast<float>(1.0 - b1);
    a.b2 = static_cast<float>(b2);
    a.omb2 = static_cast<float>(1.0 - b2);
    a.eps = static_cast<float>(eps);
    a.step_size = static_cast<float>(lr / bc1);
    a.bc2_sqrt = static_cast<float>(std::sqrt(bc2));
    a.sched = sched;
    const int grid = stream_grid(ceil_div_ll(nmax, 4), kSumsqThreads);
    return launch_adam_multi(a, grid, nspan, static_cast<hipStream_t>(stream));
}

int nr_mlp_forward(const NrMlpConfig* cfg, const void* packed, const float* params, const float* x, const float* d,
                   int64_t M, float* rgb, float* sigma, void* saved, nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(packed && params && x && rgb && sigma && M >= 0, "nr_mlp_forward: null pointer");
    NR_REQUIRE(!p.use_vd || d, "nr_mlp_forward: use_view_dirs needs d (model.py:187-191)");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(saved) & 15) == 0, "nr_mlp_forward: saved must be 16-byte aligned");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "nr_mlp_forward: packed must be 16-byte aligned");
    if (M == 0) return NR_OK;
    const MlpSizes z = make_sizes(p, M);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.prec != NR_PREC_FP32) {
        RbmArgs r{};
        fwd_io(r, p, packed, params, x, d, M, z.tiles, rgb, sigma, saved, z.saved_off, z.mask_off);
        r.base = p.lin[0].pk_fwd;
        r.vhead = p.vhead;
        return launch_fwd_rbm(p, r, saved ? FwdSave::Train : FwdSave::Infer, s);
    }
    FwdArgs a{};
    fwd_io(a, p, packed, params, x, d, M, z.tiles, rgb, sigma, saved, z.saved_off, z.mask_off);
    const char* why = "";
    NR_REQUIRE(fwd_stream(p, &a.sd, &a.slot_bytes, &why), "nr_mlp_forward: %s", why);
    for (int l = 0; l < p.n_lin; ++l) a.vb[l] = p.lin[l].vb;
    a.vsig = p.vsig;
    a.vrgb = p.vrgb;
    return launch_fwd(p, a, saved != nullptr, s);
}

int nr_mlp_backward_dx(const NrMlpConfig* cfg, const void* packed, const float* params, const float* x,
                       const float* d, int64_t M, const float* rgb, const float* sigma, const void* saved,
                       const float* g_rgb, const float* g_sigma, float* g_x, float* g_d, void* workspace,
                       nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(packed && params && x && rgb && sigma && saved && g_rgb && g_sigma && workspace && M >= 0,
               "nr_mlp_backward_dx: null pointer");
    NR_REQUIRE(!g_d || (d && p.use_vd), "nr_mlp_backward_dx: g_d needs d and use_view_dirs");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "nr_mlp_backward_dx: workspace must be 16-byte aligned");
    if (M == 0) return NR_OK;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const MlpSizes z = make_sizes(p, M);
    NR_REQUIRE(z.tiles_alloc < (int64_t{1} << 32), "nr_mlp_backward_dx: M beyond 2^37 samples");
    // the active tiles' flags (every tile with cfg->dense_backward); the dX launch
    // concatenates each segment's into the dW kernel's list (place_segment)
    char* wsb = static_cast<char*>(workspace);
    uint8_t* tflags = reinterpret_cast<uint8_t*>(wsb + z.flags_off);
    uint32_t* blkcnt = reinterpret_cast<uint32_t*>(wsb + z.blkcnt_off);
    uint32_t* dwlist = reinterpret_cast<uint32_t*>(wsb + z.dwlist_off);
    uint32_t* tcount = reinterpret_cast<uint32_t*>(wsb + z.count_off);
    if (const int rc = launch_tile_flags(g_rgb, g_sigma, M, p.dense_bwd, z.nseg, tflags, blkcnt, s)) return rc;
    const int n = p.n_layers;
    if (p.prec != NR_PREC_FP32) {
        // 16-bit: the row-block-major dX chain (mlp_bwd_rbm.inc); g_x / g_d come from a
        // separate pass over the dz images it stores (mlp_dinput_kernel)
        BwdrArgs r{};
        dx_io(r, p, packed, M, z.tiles, z.nseg, rgb, sigma, saved, z.mask_off, g_rgb, g_sigma, wsb, z.ws_off, tflags,
              blkcnt, dwlist, tcount);
        r.base = p.lin[n + 1].pk_bwdr;
        r.vhead = p.vhead;
        r.scratch_base = z.tiles_alloc - kScratchTiles;
        const int rc = launch_bwd_rbm(p, r, false, s);
        if (rc != NR_OK || !(g_x || g_d)) return rc;
        return input_grads16(p, din_offsets(p, z), r.packed, x, d, g_x, g_d, wsb, M, s);
    }
    // fp32: the chunk-major chain, which computes g_x / g_d itself when they are wanted
    const bool wx = g_x != nullptr || g_d != nullptr;
    BwdArgs b{};
    dx_io(b, p, packed, M, z.tiles, z.nseg, rgb, sigma, saved, z.mask_off, g_rgb, g_sigma, wsb, z.ws_off, tflags, blkcnt,
          dwlist, tcount);
    b.x = x;
    b.d = d;
    b.L = p.L;
    b.Ld = p.Ld;
    b.skips = p.skips;
    b.g_x = g_x;
    b.g_d = g_d;
    b.inv_gscale = 1.0f / b.gscale;
    const char* why = "";
    NR_REQUIRE(bwd_stream(p, wx, &b.sd, &b.slot_bytes, &why), "nr_mlp_backward_dx: %s", why);
    b.vsig = p.vsig;
    if (!p.dense_bwd) {
        // the chain writes g_x / g_d of the active tiles only: the rest are exactly zero
        for (float* g : {g_x, g_d})
            if (g) {
                const int64_t n = 3 * M, blocks = (n + 255) / 256;
                hipLaunchKernelGGL(zero_f32_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256),
                                   0, s, g, n);
                if (const int rc = check_launch("nr_mlp_backward_dx (zeroed input gradients)")) return rc;
            }
    }
    return launch_bwd(p, b, wx, s);
}

int nr_mlp_backward_dw(const NrMlpConfig* cfg, int64_t M, const void* saved, void* workspace, nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(saved && workspace && M >= 0, "nr_mlp_backward_dw: null pointer");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(saved) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "nr_mlp_backward_dw: saved and workspace must be 16-byte aligned");
    if (M == 0) return NR_OK;
    const MlpSizes z = make_sizes(p, M);
    NR_REQUIRE(z.max_chunks < 2048, "nr_mlp_backward_dw: %d chunks beyond the workgroup map", z.max_chunks);
    DwArgs w;  // the list and count: written by nr_mlp_backward_dx
    int nwg;
    size_t lds;
    const char* why = "";
    NR_REQUIRE(dw_args(p, z, static_cast<const char*>(saved), static_cast<char*>(workspace), &w, &nwg, &lds, &why),
               "nr_mlp_backward_dw: %s", why);
    return launch_dw(p.prec, w, nwg, lds, static_cast<hipStream_t>(stream));
}

int nr_mlp_backward_reduce(const NrMlpConfig* cfg, int64_t M, const void* workspace, float* g_params,
                           nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(workspace && g_params && M >= 0, "nr_mlp_backward_reduce: null pointer");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (M == 0) {
        (void)hipMemsetAsync(g_params, 0, sizeof(float) * p.param_count, s);
        return check_launch("nr_mlp_backward_reduce");
    }
    ReduceArgs r;
    const int max_rows = reduce_args(p, make_sizes(p, M), static_cast<const char*>(workspace), g_params, &r);
    return launch_dw_reduce(r, max_rows, s);
}

int64_t nr_mlp_frozen_saved_bytes(const NrMlpConfig* cfg, int64_t M) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p) || M < 0) return -1;
    return make_frozen_sizes(p, M).saved_bytes;
}

int64_t nr_mlp_frozen_workspace_bytes(const NrMlpConfig* cfg, int64_t M) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p) || M < 0) return -1;
    return make_frozen_sizes(p, M).ws_bytes;
}

int nr_mlp_forward_frozen(const NrMlpConfig* cfg, const void* packed, const float* params, const float* x,
                          const float* d, int64_t M, float* rgb, float* sigma, void* saved_frozen,
                          nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(packed && params && x && rgb && sigma && saved_frozen && M >= 0, "nr_mlp_forward_frozen: null pointer");
    NR_REQUIRE(!p.use_vd || d, "nr_mlp_forward_frozen: use_view_dirs needs d (model.py:187-191)");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(saved_frozen) & 15) == 0,
               "nr_mlp_forward_frozen: saved_frozen must be 16-byte aligned");
    NR_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "nr_mlp_forward_frozen: packed must be 16-byte aligned");
    if (M == 0) return NR_OK;
    // fp32: the training forward (its backward reads the activations)
    if (p.prec == NR_PREC_FP32) return nr_mlp_forward(cfg, packed, params, x, d, M, rgb, sigma, saved_frozen, stream);
    const FrozenSizes f = make_frozen_sizes(p, M);
    RbmArgs r{};
    fwd_io(r, p, packed, params, x, d, M, f.tiles, rgb, sigma, saved_frozen, nullptr, 0);
    r.base = p.lin[0].pk_fwd;
    r.vhead = p.vhead;
    return launch_fwd_rbm(p, r, FwdSave::Masks, static_cast<hipStream_t>(stream));
}

int nr_mlp_backward_input(const NrMlpConfig* cfg, const void* packed, const float* params, const float* x,
                          const float* d, int64_t M, const float* rgb, const float* sigma, const void* saved_frozen,
                          const float* g_rgb, const float* g_sigma, float* g_x, float* g_d, void* workspace,
                          nr_stream_t stream) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p)) return NR_EARG;
    NR_REQUIRE(packed && params && x && rgb && sigma && saved_frozen && g_rgb && g_sigma && workspace && M >= 0,
               "nr_mlp_backward_input: null pointer");
    NR_REQUIRE(!g_d || (d && p.use_vd), "nr_mlp_backward_input: g_d needs d and use_view_dirs");
    NR_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(saved_frozen)) & 15) == 0,
               "nr_mlp_backward_input: saved_frozen and workspace must be 16-byte aligned");
    if (M == 0 || !(g_x || g_d)) return NR_OK;
    // fp32: the dx stage of the training backward, which computes g_x / g_d itself
    if (p.prec == NR_PREC_FP32)
        return nr_mlp_backward_dx(cfg, packed, params, x, d, M, rgb, sigma, saved_frozen, g_rgb, g_sigma, g_x, g_d,
                                  workspace, stream);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const FrozenSizes f = make_frozen_sizes(p, M);
    NR_REQUIRE(f.tiles + kScratchTiles < (int64_t{1} << 32), "nr_mlp_backward_input: M beyond 2^37 samples");
    char* wsb = static_cast<char*>(workspace);
    uint8_t* tflags = reinterpret_cast<uint8_t*>(wsb + f.flags_off);
    uint32_t* blkcnt = reinterpret_cast<uint32_t*>(wsb + f.blkcnt_off);
    if (const int rc = launch_tile_flags(g_rgb, g_sigma, M, p.dense_bwd, f.nseg, tflags, blkcnt, s)) return rc;
    // the dz images the input-only chain stores, by workspace tensor id; no dW list
    int64_t ws_off[kMaxTrunk + 3] = {};
    for (int l = 0; l < p.n_layers; ++l) ws_off[WS_DZ0 + l] = f.dz_off[l];
    ws_off[p.ws_dir] = f.dz_dir_off;
    BwdrArgs r{};
    dx_io(r, p, packed, M, f.tiles, f.nseg, rgb, sigma, saved_frozen, 0, g_rgb, g_sigma, wsb, ws_off, tflags, blkcnt,
          nullptr, nullptr);
    r.base = p.lin[p.n_layers + 1].pk_bwdr;
    r.vhead = p.vhead;
    r.scratch_base = f.scratch_base;
    r.keep_dz = f.keep_dz;
    if (const int rc = launch_bwd_rbm(p, r, true, s)) return rc;
    return input_grads16(p, din_offsets(p, f), r.packed, x, d, g_x, g_d, wsb, M, s);
}

int64_t nr_mlp_active_tiles_offset(const NrMlpConfig* cfg, int64_t M) {
    MlpPlan p;
    if (!plan_or_error(cfg, &p) || M <= 0) return -1;
    return make_sizes(p, M).count_off;
}

int nr_mlp_backward(const NrMlpConfig* cfg, const void* packed, const float* params, const float* x, const float* d,
                    int64_t M, const float* rgb, const float* sigma, const void* saved, const float* g_rgb,
                    const float* g_sigma, float* g_params, float* g_x, float* g_d, void* workspace,
                    nr_stream_t stream) {
    NR_REQUIRE(g_params, "nr_mlp_backward: null g_params");
    // the split form: dX chain (dz images), then the dW GEMM over them
    int rc = nr_mlp_backward_dx(cfg, packed, params, x, d, M, rgb, sigma, saved, g_rgb, g_sigma, g_x, g_d, workspace,
                                stream);
    if (rc) return rc;
    rc = nr_mlp_backward_dw(cfg, M, saved, workspace, stream);
    if (rc) return rc;
    return nr_mlp_backward_reduce(cfg, M, workspace, g_params, stream);
}

}  // extern "C"


// Between mlp.hip (the extern "C" entry points, which fill these argument structs from
// the plan) and the translation units that hold the kernels and launch them.  The
// descriptors that are functions of the plan alone (StreamDesc, DwArgs, ReduceArgs) and
// their builders are host-only code in mlp_plan.hpp; what needs HIP types is here.
#pragma once

#include <type_traits>

#include "common.hpp"
#include "mlp_plan.hpp"
#include "optim.hpp"

#pragma GCC visibility push(hidden)  // the launchers are internal to the library
namespace nr {

// ------------------------------------------- fp32, chunk-major (mlp_fp32.hip) ----
// What every forward chain reads and writes.  fwd_io() (mlp.hip) is the one place that
// assigns these fields, in whichever argument struct holds them: the 16-bit structs derive
// from the block, the fp32 structs restate its fields in an order of their own (below).
struct FwdIO {
    const char* packed;
    const float* params;
    const float* x;
    const float* d;
    float* rgb;
    float* sigma;
    char* saved;
    int64_t M, tiles;
    int L, Ld, n_layers;
    uint32_t skips;
    int64_t sig_b, rgb_b;
    int64_t sv_off[kMaxTrunk + 4];
    int sv_feat, sv_denc, sv_hc;
    int64_t mask_off;
    int n_mask;
};

// What every dX chain reads and writes; assigned by dx_io() (mlp.hip) alone.
struct DxIO {
    float gscale;               // loss scale applied to dL/d(rgb, sigma) (fp32, bf16: 1)
    const char* packed;
    const float* rgb;
    const float* sigma;
    const float* g_rgb;
    const float* g_sigma;
    const char* saved;
    char* ws;
    int64_t M, tiles;
    const uint8_t* flags;       // active tiles (tile_flags_kernel) and their 64-tile block counts
    const uint32_t* blk_count;
    int64_t nseg;
    uint32_t* dw_list;          // the dW kernel's list and count (place_segment)
    uint32_t* count;
    int n_layers;
    int64_t vrgb;
    int64_t mask_off;
    int n_mask;
    int64_t ws_off[kMaxTrunk + 3];
    int ws_feat, ws_dir, ws_heads;
};

// The fp32 kernels spill scalar registers by the hundred, and how many depends on the order
// of their argument fields (the compiler loads kernel arguments in address order): with the
// shared block first, three instances spill differently and one takes four more VGPRs.  So
// these two structs are flat, FwdIO's / DxIO's fields by the same names interleaved with
// their own in the order below, and the fillers are templates over the struct.
struct FwdArgs {
    const char* packed;
    const float* params;
    const float* x;
    const float* d;
    float* rgb;
    float* sigma;
    char* saved;
    int64_t M, tiles;
    int L, Ld, n_layers;
    uint32_t skips;
    int slot_bytes;
    StreamDesc sd;  // W images: trunk 0..n-1, feat, dir
    int64_t vb[kMaxMfmaLayers];  // bias vector images (the kernel reads no bias from params)
    int64_t vsig, vrgb, sig_b, rgb_b;
    int64_t sv_off[kMaxTrunk + 4];
    int sv_feat, sv_denc, sv_hc;
    int64_t mask_off;
    int n_mask;
};

struct BwdArgs {
    float gscale, inv_gscale;  // inv_gscale divides the loss scale out of g_x / g_d
    const char* packed;
    const float* x;            // the forward's inputs, for g_x / g_d
    const float* d;
    const float* rgb;
    const float* sigma;
    const float* g_rgb;
    const float* g_sigma;
    float* g_x;
    float* g_d;
    const char* saved;
    char* ws;
    int64_t M, tiles;
    const uint8_t* flags;
    const uint32_t* blk_count;
    int64_t nseg;
    uint32_t* dw_list;
    uint32_t* count;
    int L, Ld, n_layers;
    uint32_t skips;
    int slot_bytes;
    StreamDesc sd;  // W^T images: dir, feat, trunk n-1..1 [, trunk 0 when g_x/g_d]
    int64_t vsig, vrgb;
    int64_t mask_off;
    int n_mask;
    int64_t ws_off[kMaxTrunk + 3];
    int ws_feat, ws_dir, ws_heads;
};

// train: save the activations; want_x: also compute g_x / g_d.  a.sd and a.slot_bytes are
// fwd_stream's / bwd_stream's (mlp_plan.hpp).
int launch_fwd(const MlpPlan& p, const FwdArgs& a, bool train, hipStream_t s);
int launch_bwd(const MlpPlan& p, const BwdArgs& a, bool want_x, hipStream_t s);

// ------------------------------------- 16-bit, row-block major (mlp_16.hip) ----
struct RbmArgs : FwdIO {
    int64_t base;   // byte offset of layer 0's row-block-major image in packed
    int64_t vhead;
};

struct BwdrArgs : DxIO {
    int64_t base;           // pk_bwdr of the dir layer: the stream's first chunk
    int64_t vhead;
    int64_t scratch_base;   // first of the kScratchTiles tiles waves without an active tile run on
    uint32_t keep_dz;       // input-only chain: bit l set <=> trunk layer l's dz image is stored
};

// Infer: nothing saved.  Train: the activations and ReLU masks.  Masks: the frozen field's
// forward (FrozenSizes, mlp_plan.hpp), which stores the masks alone (a.saved = the mask
// region, a.mask_off = 0).
enum class FwdSave { Infer, Train, Masks };
int launch_fwd_rbm(const MlpPlan& p, const RbmArgs& a, FwdSave save, hipStream_t s);
// input_only: the frozen field's dX chain, which stores only the dz images of a.keep_dz and
// dz_c and builds no dW list
int launch_bwd_rbm(const MlpPlan& p, const BwdrArgs& a, bool input_only, hipStream_t s);
// g_x / g_d from the dz images the dX chain stored (mlp_dinput_kernel)
int input_grads16(const MlpPlan& p, const DinOffsets& o, const char* packed, const float* x, const float* d,
                  float* g_x, float* g_d, const char* ws, int64_t M, hipStream_t s);

// The kernels are compiled for these (XB, DB); dev builds (NR_MLP_DEV: register / ISA
// inspection) for the default model only.  Calls f(XB, DB) as std::integral_constants for
// p's instance; false when there is none (the caller words the error).
template <class F>
bool dispatch_model(const MlpPlan& p, F&& f) {
    auto at = [&](auto xb, auto db) {
        if (p.XB != xb || p.DB != db) return false;
        f(xb, db);
        return true;
    };
    using std::integral_constant;
    if (at(integral_constant<int, 2>{}, integral_constant<int, 1>{})) return true;
#ifndef NR_MLP_DEV
    if (at(integral_constant<int, 2>{}, integral_constant<int, 0>{})) return true;
    if (at(integral_constant<int, 1>{}, integral_constant<int, 1>{})) return true;
    if (at(integral_constant<int, 1>{}, integral_constant<int, 0>{})) return true;
#endif
    return false;
}

// f(PREC) for the 16-bit precision `prec`, as a std::integral_constant
template <class F>
auto dispatch_prec16(int prec, F&& f) {
    return prec == NR_PREC_BF16 ? f(std::integral_constant<int, NR_PREC_BF16>{})
                                : f(std::integral_constant<int, NR_PREC_FP16>{});
}

// --------------------------------------- active tiles, dW, reduce (mlp_dw.hip) ----
int launch_tile_flags(const float* g_rgb, const float* g_sigma, int64_t M, int dense, int64_t nseg, uint8_t* flags,
                      uint32_t* blk_count, hipStream_t s);
int launch_dw(int prec, const DwArgs& a, int nwg, size_t lds, hipStream_t s);
int launch_dw_reduce(const ReduceArgs& a, int max_rows, hipStream_t s);

// ------------------------------------ pack, fused optimizer step (mlp_pack.hip) ----
// Destination table of the fused optimizer step (see mlp_pack.hip)
constexpr int kPackSlots = 3;
constexpr int64_t kDstMaxOff = int64_t(1) << 29;
struct PackIdx {
    uint32_t* table;
    int64_t n;  // flat parameters
};

struct AdamSpanDev {
    float *p, *g, *m, *v;
    int64_t n;
    const float* partials;
    float max_norm;
    const uint32_t* table;
    char* packed;
};
struct AdamMultiArgs {
    AdamSpanDev s[kMaxAdamSpans];
    float omb1, b2, omb2, eps, step_size, bc2_sqrt;
    const float* sched;  // nullable: {step_size, bc2_sqrt} read on the device (graph replay)
};

// nr_mlp_pack's four kernels; idx: their index mode, filling the destination table
int launch_pack(const MlpPlan& p, const float* params, void* packed, PackIdx t, bool idx, hipStream_t s);
int launch_adam_multi(const AdamMultiArgs& a, int grid, int nspan, hipStream_t s);
// positional-encoding window (w_pos: L floats, w_dir: Ld floats, device, nullable = ones):
// the images' encoding columns rewritten from params times the window, and the flat
// gradient's encoding columns times it
int launch_fold_window(const MlpPlan& p, const float* params, void* packed, const float* w_pos, const float* w_dir,
                       hipStream_t s);
int launch_window_grad(const MlpPlan& p, const float* w_pos, const float* w_dir, float* g_params, hipStream_t s);

}  // namespace nr
#pragma GCC visibility pop

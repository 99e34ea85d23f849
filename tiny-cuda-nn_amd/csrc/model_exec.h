// model_exec.h -- running a described model: the encoding / network passes over the kernel launchers.  Everything a pass depends on
// is in its argument list: the stream, the trainer's profiler (null: none), the model and the layout of the caller's matrices.
#pragma once
#include <vector>

#include "composite_kernels.h"
#include "model_desc.h"
#include "profiler.h"
#include "scratch_cache.h"

namespace tcnn_hip {

// Layout of the caller's fp32 input / dL_dinput matrices (GPUMatrixDynamic: row- or column-major with a stride,
// gpu_matrix.h:106-250).  The plain entry points pass dense column-major matrices (one sample's values contiguous); the
// *_matrices entry points describe the caller's (layout_of, api_trainer.hip).
struct IoLayout {
	uint32_t in_stride_i, in_stride_d;  // input element (sample i, dim d) at [i * in_stride_i + d * in_stride_d]
	uint32_t dx_stride_i, dx_stride_d;  // the same for dL_dinput
	static IoLayout dense(const Model& md) { return {md.n_input_dims, 1u, md.n_input_dims, 1u}; }
};

struct ForwardCtx {
	hipStream_t stream = nullptr;
	uint32_t n = 0;
	Scratch enc;     // half, feature-major [enc.padded][n]   (network_with_input_encoding.h:76)
	Scratch hidden;  // half [n_hidden][n][width]             (fully_fused_mlp.cu:841-854)
	Scratch dy_dx;   // fp32 [(k*n + i)*D + d]                (grid.h:783-785)
	// Composite encoding (composite.h:226-233): the matrix the Sum / Product reduction read (the product's backward needs it), in the value
	// type and layout of the pass's output with unreduced_width() rows; one dy_dx per nested encoding (allocated for the grids)
	Scratch unreduced;
	std::vector<Scratch> nested_dy_dx;
	// a lone grid's max_level state as the forward pass that filled this context read it: the backward and second-order passes of the context
	// run with these, whatever the setters have been told since (EncodingDesc::max_level_gpu says whose memory the array is)
	float max_level = 1.0f;
	const float* max_level_gpu = nullptr;
	// filled by a *_half_input forward pass (the caller's 16-bit matrix stood where the fp32 one stands): the backward pass of this context is
	// the *_half_input one, and the other way round
	bool half_input = false;
	void keep_max_level(const EncodingDesc& e) {
		max_level = e.grid.max_level;
		max_level_gpu = e.max_level_gpu;
	}
};

// The grid's parameter gradients in groups of consecutive levels, each reported as soon as its kernels are enqueued (data-parallel
// hosts start that group's exchange while the next group is still being computed): `ready(ctx, begin, end)` with the parameter range
// relative to the model's first parameter.
struct LevelGroups {
	uint32_t n_groups = 1;
	void (*ready)(void* ctx, size_t begin, size_t end) = nullptr;
	void* ctx = nullptr;
};
// The C ABI's max_level entry points (api_module.hip, api_trainer.hip): TCNN_OK where `md` has a lone top-level grid, otherwise the last error
// is set to Model::max_level_refusal() and TCNN_ERROR_UNSUPPORTED comes back
int refuse_max_level(const Model& md);
void check_batch(uint32_t n, uint32_t widest = 128);
uint32_t widest_matrix(const Model& md);  // the widest matrix any pass over `md` indexes, in elements per sample

// One grid's slice of a pass, the same for a lone grid and for one nested in a Composite: positions from input dim dims_to_encode_begin on; the
// encoded matrix (or dL_dy) as the grid sees it, i.e. the caller hands the kernels its matrix from row output_row on.  A lone grid also carries
// its max_level state (the encoding's own in a forward pass, the context's in every pass behind it); nested grids have none.
struct GridSlice {
	GridMeta grid;
	GridIO io;
	GridSlice& max_level(float value, const float* per_sample) {
		grid.max_level = value;
		io.max_level = per_sample;
		return *this;
	}
};
inline GridSlice grid_slice(const EncodingDesc& g, const IoLayout& layout, const float* input, uint32_t n, uint32_t stride_k, uint32_t stride_i) {
	return {g.grid, {input + (size_t)g.dims_to_encode_begin * layout.in_stride_d, layout.in_stride_i, layout.in_stride_d, n, stride_k, stride_i}};
}
// grid_backward reports its kernels one by one (GridBackwardWorkspace::phase_hook): the pass's timer, for the profiler's two backward stages
struct PhaseTimer {
	Profiler* profiler;
	hipStream_t stream;
	bool counts = true;  // false once the step's first launch sequence is out: later ones (level groups, further grids) add time, not launches
	hipEvent_t a = nullptr;  // the open phase's first event
};
// The 16-bit parameter gradients of one grid slice: takes the backward's workspace (scratch, zeroed counters, the timer's hook) and runs
// grid_backward.  With `groups` the levels go in ranges -- one workspace, sized to the largest -- and `ready` is called per range, the
// parameter range counted from `first_param`.
void grid_backward_with_workspace(hipStream_t stream, const GridSlice& s, const half_t* dL_dy, half_t* grid_gradient, bool accumulate, GridBackwardMode mode,
                                  uint32_t lds_level_budget, PhaseTimer* timer = nullptr, const LevelGroups* groups = nullptr, size_t first_param = 0);

// What the caller of a pass states first, once: the batch guards (false: an empty batch, nothing to do).  A forward pass files the batch in
// its context (stream, n, the lone grid's max_level state); a backward pass checks the batch against the context it was given.
bool begin_pass(hipStream_t stream, const Model& md, uint32_t n, ForwardCtx* ctx = nullptr);
bool begin_backward(const Model& md, const ForwardCtx& ctx, uint32_t n);
// Encoding forward, T = the 16-bit type or float (Encoding<float>, which computes in fp32): `out` has element (feature k, sample i) at
// [k * stride_k + i * stride_i] -- feature-major (stride_k = n, stride_i = 1) in front of a network, sample-major (1, padded width) bare.
// Leaves in `ctx` (null: inference) what the backward pass needs: dy_dx when prepare_input_gradients is set, a Composite's unreduced
// matrix.  The caller has been through begin_pass (model_forward, the trainer's fused step, the fp32 module entries).
template <typename T>
void encoding_forward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const T* enc_params, T* out,
                      uint32_t stride_k, uint32_t stride_i, ForwardCtx* ctx = nullptr, bool prepare_input_gradients = false);
// the encoding's share of the backward pass: dL_denc has element (feature k, sample i) at [k * stride_k + i * stride_i]; dL_dparams is the
// model's (the encoding's behind the network's).  The fp32 grid backward has one formulation: budget and groups are the 16-bit one's.
// The caller has been through begin_backward (model_backward, the fp32 module entry) or made `ctx` itself in this call (the fused step).
template <typename T>
void encoding_backward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const T* dL_denc,
                       uint32_t stride_k, uint32_t stride_i, T* dL_dparams, bool want_grads, bool accumulate, const float* input,
                       uint32_t lds_level_budget = 0, const LevelGroups* groups = nullptr);
// The caller's own 16-bit input / dL_dinput matrices (tcnn_module_*_half_input; dense [n][n_input_dims] in the library's 16-bit type) go to
// exactly the modules tcnn_create_network makes: a network behind an Identity encoding with scale 1 and offset 0, which is exact on values of
// that type.  Why `md` is not one of them (empty: it is); refuse_half_input sets that as the last error and returns TCNN_ERROR_UNSUPPORTED.
std::string half_input_refusal(const Model& md);
int refuse_half_input(const Model& md);
// NetworkWithInputEncoding::forward_impl / inference_mixed_precision_impl (:60-81).  ctx == nullptr: inference.
// input16 (only where half_input_refusal(md) is empty; `input` is then ignored): half_input_pad writes the encoded matrix from it.
void model_forward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, uint32_t n, const float* input, half_t* output, const half_t* params,
                   ForwardCtx* ctx, bool prepare_input_gradients, const MlpF32Output* f32 = nullptr, const half_t* input16 = nullptr);
// NetworkWithInputEncoding::backward_impl (:83-113) / GridEncodingTemplated::backward_impl (grid.h:817-908)
void model_backward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const half_t* dL_doutput,
                    half_t* dL_dparams, const float* input, const half_t* output, const half_t* params, int gradient_mode,
                    uint32_t lds_level_budget, half_t* dL_dinput16 = nullptr);  // dL_dinput16: of a context made with input16, instead of dL_dinput
// The same two passes of a model whose network is the fp32 one (NetworkDesc::fp32, mlp_kernels.h mlp_f32_*): parameters, output, dL_doutput and
// dL_dparams are float, the encoding runs its fp32 path (encoding_forward<float> / encoding_backward<float>) and hands the network an fp32
// feature-major matrix; the context keeps that matrix and the saved fp32 activations.  trimmed (inference only, ctx == nullptr): the result
// goes to the caller's trimmed matrix instead of `output`.
void model_forward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, float* output, const float* params, ForwardCtx* ctx,
                       bool prepare_input_gradients, const MlpF32Output* trimmed = nullptr);
void model_backward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const float* dL_doutput, float* dL_dparams,
                        const float* input, const float* output, const float* params, int gradient_mode);
// The second-order pass (backward_backward_input) of the modules tcnn_create_network_precision(..., TCNN_PRECISION_FP32) makes -- an fp32
// network behind the Identity encoding with scale 1 and offset 0, which fp32_second_order_network tells: the gradients of
// <dL_ddLdinput, dL_dinput> with respect to dL_doutput ([n][padded outputs]), the parameters (overwritten) and the input ([n][n_input_dims]).
// Each result may be null; dL_doutput is needed for the last two.  `ctx` is the forward pass's (encoded input, saved activations).
bool fp32_second_order_network(const Model& md);
void model_backward_backward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, const float* dL_ddLdinput, const float* dL_doutput,
                                 float* dL_dparams, float* dL_ddLdoutput, float* dL_dinput, const float* params);
// network->inference into the caller's fp32 matrix (object.h:214-271)
void inference_to_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const half_t* params, float* out, uint32_t stride_i, uint32_t stride_j);

}  // namespace tcnn_hip

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
// Encoding forward into a feature-major (SoA) or sample-major (AoS) half matrix.  dy_dx: a lone grid's; a Composite keeps what its backward
// pass needs in `ctx` (null: inference), its nested grids' dy_dx when prepare_input_gradients is set.
void encoding_forward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const half_t* enc_params, half_t* out,
                      bool soa, float* dy_dx, ForwardCtx* ctx = nullptr, bool prepare_input_gradients = false);
// the encoding's share of the backward pass: dL_denc has element (feature k, sample i) at [k * stride_k + i * stride_i]
void encoding_backward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const half_t* dL_denc,
                       uint32_t stride_k, uint32_t stride_i, half_t* dL_dparams, bool want_grads, bool accumulate, const float* input,
                       uint32_t lds_level_budget, const LevelGroups* groups = nullptr);
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
// network->inference into the caller's fp32 matrix (object.h:214-271)
void inference_to_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const half_t* params, float* out, uint32_t stride_i, uint32_t stride_j);
// Encoding<float>: a bare encoding that computes in fp32 (model_exec.hip)
void encoding_forward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const float* params, float* out, ForwardCtx* ctx,
                          bool prepare_input_gradients);
void encoding_backward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const float* dL_doutput, float* dL_dparams,
                           const float* input);

}  // namespace tcnn_hip

// api_module.hip -- C ABI: the type-erased Module (tcnn_module_*; reference src/cpp_api.cu:72-174) over model_desc / model_exec.
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "host_common.h"
#include "model_exec.h"
#include "switches.h"

using namespace tcnn_hip;

struct tcnn_module {
	Model md;
	std::string name;
	uint32_t lds_level_budget = 0;  // 0: default LDS slice size of the sliced grid backward
	// create_encoding(..., Precision::Fp32) (cpp_api.cu:165-174 -> Encoding<float>): parameters, outputs and gradients are fp32 and the
	// first-order passes COMPUTE in fp32 (encoding_forward<float> / encoding_backward<float>: the grid's kernel_grid<float> formulation, fp32
	// global atomics for its parameter gradients; frequency / one-blob / identity with float values).  So does the second-order pass
	// (backward_backward_input, grid only): the T = float instances of the reference's three kernels on the caller's own tensors.
	// tcnn_set_fp32_second_order(1) brings back the 16-bit stand-ins it used to run on (A/B runs, tests): incoming gradients are scaled
	// into that type's range by the largest power of two <= FP32_GRADIENT_SCALE that keeps max |dL_doutput| * scale <=
	// FP32_GRADIENT_TARGET (found on the device per call) and the results scaled back, exactly.
	bool fp32_io = false;
	// tcnn_create_network[_with_input_encoding]_precision(..., TCNN_PRECISION_FP32): the network is the fp32 layer-by-layer one
	// (NetworkDesc::fp32, mlp_kernels.h mlp_f32_*) behind the encoding's fp32 path; fp32_io is set as well (precisions, no 16-bit inputs)
	bool fp32_network() const { return fp32_io && md.has_network; }
};
static constexpr float FP32_GRADIENT_SCALE = 1024.0f, FP32_GRADIENT_TARGET = 16384.0f;
// the 16-bit copies an fp32 module works on with tcnn_set_fp32_second_order(1)
struct Fp32Bridge {
	Scratch params, output, dL_doutput, dL_dparams;
	static Scratch to_half(hipStream_t stream, const void* src, size_t n, float scale = 1.0f) {
		Scratch s(stream, std::max<size_t>(n, 1) * sizeof(half_t));
		cast_scaled_f32_to_f16(stream, n, (const float*)src, s.as<half_t>(), scale);
		return s;
	}
	// the gradient entering the backward pass: scaled by a per-call power of two left in `scale_pair` ({scale, 1 / scale} on the device)
	static Scratch gradient_to_half(hipStream_t stream, const void* src, size_t n, Scratch& scale_pair) {
		scale_pair = Scratch(stream, 4 * sizeof(float));
		gradient_scale_from_absmax(stream, n, (const float*)src, scale_pair.as<float>(), FP32_GRADIENT_SCALE, FP32_GRADIENT_TARGET);
		Scratch s(stream, std::max<size_t>(n, 1) * sizeof(half_t));
		cast_scaled_f32_to_f16(stream, n, (const float*)src, s.as<half_t>(), (const float*)scale_pair.as<float>());
		return s;
	}
};
struct tcnn_context {
	ForwardCtx ctx;
};

extern "C" {

int tcnn_create_network_with_input_encoding(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json, const char* network_json,
                                            tcnn_module_t** out) {
	TCNN_API_BEGIN
	auto m = std::make_unique<tcnn_module>();
	m->md = make_nwie(n_input_dims, n_output_dims, Json::parse(encoding_json), Json::parse(network_json));
	m->name = m->md.name();
	*out = m.release();
	TCNN_API_END
}

int tcnn_create_network(uint32_t n_input_dims, uint32_t n_output_dims, const char* network_json, tcnn_module_t** out) {
	return tcnn_create_network_with_input_encoding(n_input_dims, n_output_dims, "{\"otype\": \"Identity\"}", network_json, out);  // cpp_api.cu:160-162
}

// The two creators above with create_encoding's `requested_precision`: the library's own 16-bit precision gives exactly their modules;
// TCNN_PRECISION_FP32 an fp32 network (CutlassMLP under every spelling: the reference without half precision, network.cu:51-138) behind the
// encoding's fp32 path.
int tcnn_create_network_with_input_encoding_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json, const char* network_json,
                                                      int requested_precision, tcnn_module_t** out) {
	if (requested_precision == NATIVE_PRECISION) return tcnn_create_network_with_input_encoding(n_input_dims, n_output_dims, encoding_json, network_json, out);
	TCNN_API_BEGIN
	if (requested_precision != TCNN_PRECISION_FP32) {
		set_last_error(HALF_IS_BF16 ? "create_network: this build (libtcnn_hip_bf16.so) provides bf16 and fp32 networks" : "create_network: this build provides fp16 and fp32 networks");
		return TCNN_ERROR_UNSUPPORTED;
	}
	auto m = std::make_unique<tcnn_module>();
	m->fp32_io = true;
	m->md = make_nwie(n_input_dims, n_output_dims, Json::parse(encoding_json), Json::parse(network_json), /*fp32_network=*/true);
	m->name = m->md.name();
	*out = m.release();
	TCNN_API_END
}

int tcnn_create_network_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* network_json, int requested_precision, tcnn_module_t** out) {
	return tcnn_create_network_with_input_encoding_precision(n_input_dims, n_output_dims, "{\"otype\": \"Identity\"}", network_json, requested_precision, out);
}

// create_from_config with a requested precision: the trainer is 16-bit only (its fused loss and optimizer launches have no fp32 path)
int tcnn_create_from_config_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* config_json, uint32_t seed, int requested_precision,
                                      tcnn_trainable_model_t** out) {
	if (requested_precision == NATIVE_PRECISION) return tcnn_create_from_config(n_input_dims, n_output_dims, config_json, seed, out);
	set_last_error(requested_precision == TCNN_PRECISION_FP32
	                   ? "create_from_config: the trainer (tcnn_create_from_config, training_step and the data-parallel entry points on it) is 16-bit only in this build; "
	                     "fp32 networks are modules (tcnn_create_network_precision / tcnn_create_network_with_input_encoding_precision)"
	                   : "create_from_config: this build's trainer runs in the library's own 16-bit precision only");
	return TCNN_ERROR_UNSUPPORTED;
}

int tcnn_create_encoding(uint32_t n_input_dims, const char* encoding_json, int requested_precision, tcnn_module_t** out) {
	TCNN_API_BEGIN
	if (requested_precision != NATIVE_PRECISION && requested_precision != TCNN_PRECISION_FP32) {
		set_last_error(HALF_IS_BF16 ? "create_encoding: this build (libtcnn_hip_bf16.so) provides bf16 and fp32 encodings"
		                            : "create_encoding: this build provides fp16 and fp32 encodings");
		return TCNN_ERROR_UNSUPPORTED;
	}
	auto m = std::make_unique<tcnn_module>();
	m->fp32_io = requested_precision == TCNN_PRECISION_FP32;
	m->md.n_input_dims = n_input_dims;
	m->md.enc = create_encoding_desc(n_input_dims, Json::parse(encoding_json), /*alignment=*/0);  // cpp_api.cu:165-174
	m->md.has_network = false;
	m->md.finish();
	m->name = m->md.name();
	*out = m.release();
	TCNN_API_END
}

void tcnn_module_destroy(tcnn_module_t* m) { delete m; }

int tcnn_module_inference(tcnn_module_t* m, tcnn_stream_t stream_, uint32_t n, const float* input, void* output, void* params) {
	TCNN_API_BEGIN
	hipStream_t stream = (hipStream_t)stream_;
	if (m->fp32_network()) {
		model_forward_f32(stream, m->md, IoLayout::dense(m->md), n, input, (float*)output, (const float*)params, nullptr, false);
		return TCNN_OK;
	}
	if (m->fp32_io) {
		if (begin_pass(stream, m->md, n)) encoding_forward(stream, nullptr, m->md, IoLayout::dense(m->md), n, input, (const float*)params, (float*)output, 1u, m->md.enc.padded_output_width);
		return TCNN_OK;
	}
	model_forward(stream, nullptr, m->md, IoLayout::dense(m->md), n, input, (half_t*)output, (const half_t*)params, nullptr, false);
	TCNN_API_END
}

int tcnn_module_forward(tcnn_module_t* m, tcnn_stream_t stream_, uint32_t n, const float* input, void* output, void* params,
                        int prepare_input_gradients, tcnn_context_t** ctx) {
	TCNN_API_BEGIN
	hipStream_t stream = (hipStream_t)stream_;
	auto c = std::make_unique<tcnn_context>();
	if (m->fp32_network()) {
		model_forward_f32(stream, m->md, IoLayout::dense(m->md), n, input, (float*)output, (const float*)params, &c->ctx, prepare_input_gradients != 0);
	} else if (m->fp32_io) {
		if (begin_pass(stream, m->md, n, &c->ctx)) {
			encoding_forward(stream, nullptr, m->md, IoLayout::dense(m->md), n, input, (const float*)params, (float*)output, 1u, m->md.enc.padded_output_width, &c->ctx,
			                 prepare_input_gradients != 0);
		}
	} else {
		model_forward(stream, nullptr, m->md, IoLayout::dense(m->md), n, input, (half_t*)output, (const half_t*)params, &c->ctx, prepare_input_gradients != 0);
	}
	*ctx = c.release();
	TCNN_API_END
}

// backward with the gradient mode spelled out (GradientMode, common.h:152-156): dL_dparams is overwritten, accumulated into, or left alone
int tcnn_module_backward_gradient_mode(tcnn_module_t* m, tcnn_stream_t stream, const tcnn_context_t* ctx, uint32_t n, float* dL_dinput, const void* dL_doutput,
                                       void* dL_dparams, const float* input, const void* output, const void* params, int gradient_mode) {
	TCNN_API_BEGIN
	if (!m) throw std::runtime_error("backward: null module");
	if (!ctx) throw std::runtime_error("backward: missing forward context");
	if (gradient_mode != TCNN_GRADIENT_IGNORE && gradient_mode != TCNN_GRADIENT_OVERWRITE && gradient_mode != TCNN_GRADIENT_ACCUMULATE) throw std::runtime_error("backward: invalid gradient mode");
	if (ctx->ctx.half_input) throw std::runtime_error("backward: this context was made by tcnn_module_forward_half_input; its backward pass is tcnn_module_backward_half_input");
	if (!dL_dparams) gradient_mode = TCNN_GRADIENT_IGNORE;
	if (m->fp32_network()) {
		model_backward_f32((hipStream_t)stream, m->md, IoLayout::dense(m->md), ctx->ctx, n, dL_dinput, (const float*)dL_doutput, (float*)dL_dparams, input, (const float*)output,
		                   (const float*)params, gradient_mode);
		return TCNN_OK;
	}
	if (m->fp32_io) {  // bare encodings: neither `output` nor the parameters are needed by their first-order backward pass
		if (begin_backward(m->md, ctx->ctx, n)) {
			encoding_backward((hipStream_t)stream, nullptr, m->md, IoLayout::dense(m->md), ctx->ctx, n, dL_dinput, (const float*)dL_doutput, 1u, m->md.enc.padded_output_width,
			                  (float*)dL_dparams, gradient_mode != TCNN_GRADIENT_IGNORE, gradient_mode == TCNN_GRADIENT_ACCUMULATE, input);
		}
		return TCNN_OK;
	}
	model_backward((hipStream_t)stream, nullptr, m->md, IoLayout::dense(m->md), ctx->ctx, n, dL_dinput, (const half_t*)dL_doutput, (half_t*)dL_dparams, input, (const half_t*)output,
	               (const half_t*)params, gradient_mode, m->lds_level_budget);
	TCNN_API_END
}

int tcnn_module_backward(tcnn_module_t* m, tcnn_stream_t stream, const tcnn_context_t* ctx, uint32_t n, float* dL_dinput, const void* dL_doutput,
                         void* dL_dparams, const float* input, const void* output, const void* params) {
	return tcnn_module_backward_gradient_mode(m, stream, ctx, n, dL_dinput, dL_doutput, dL_dparams, input, output, params, TCNN_GRADIENT_OVERWRITE);  // cpp_api.cu:115
}

// network->inference of a module (object.h:214-271): into the caller's fp32 matrix of n_output_dims (unpadded) x n, either layout
int tcnn_module_inference_matrix(tcnn_module_t* m, tcnn_stream_t stream_, uint32_t n, const float* input, const tcnn_matrix_t* output, const void* params) {
	TCNN_API_BEGIN
	if (!m || !output) throw std::runtime_error("tcnn_module_inference_matrix: null argument");
	if (!m->md.has_network) {
		set_last_error(std::string("inference_matrix: ") + m->md.enc.name() + " is a bare encoding; its inference is tcnn_module_inference");
		return TCNN_ERROR_UNSUPPORTED;
	}
	const uint32_t width = m->md.output_width();
	if (output->m != width || output->n != n || !output->data) throw std::runtime_error("inference_matrix: the output matrix must be n_output_dims x n_elements");
	const bool cm = output->layout == TCNN_LAYOUT_COLUMN_MAJOR;
	if (!cm && output->layout != TCNN_LAYOUT_ROW_MAJOR) throw std::runtime_error("inference_matrix: invalid layout");
	if (output->stride < (cm ? width : n)) throw std::runtime_error("inference_matrix: the stride is below the leading dimension");
	const uint32_t stride_i = cm ? output->stride : 1u, stride_j = cm ? 1u : output->stride;
	hipStream_t stream = (hipStream_t)stream_;
	if (m->fp32_network()) {
		const MlpF32Output trimmed = {(float*)output->data, width, stride_i, stride_j};
		model_forward_f32(stream, m->md, IoLayout::dense(m->md), n, input, nullptr, (const float*)params, nullptr, false, &trimmed);
		return TCNN_OK;
	}
	check_batch(n, widest_matrix(m->md));
	inference_to_f32(stream, m->md, IoLayout::dense(m->md), n, input, (const half_t*)params, (float*)output->data, stride_i, stride_j);
	TCNN_API_END
}

// ---- the same three with the caller's own 16-bit input / dL_dinput matrices ([n][n_input_dims] dense, fp16 -- bf16 in libtcnn_hip_bf16.so), for
// the modules tcnn_create_network makes (model_exec.h half_input_refusal): no fp32 copy of a matrix that a 16-bit producer wrote and the
// network reads in 16 bits anyway.  Same bits as the fp32 entries on the widened matrix.
int tcnn_module_supports_half_input(const tcnn_module_t* m) { return m && !m->fp32_io && half_input_refusal(m->md).empty() ? 1 : 0; }

int tcnn_module_inference_half_input(tcnn_module_t* m, tcnn_stream_t stream, uint32_t n, const void* input, void* output, void* params) {
	TCNN_API_BEGIN
	if (!m) throw std::runtime_error("tcnn_module_inference_half_input: null module");
	if (const int r = refuse_half_input(m->md)) return r;
	model_forward((hipStream_t)stream, nullptr, m->md, IoLayout::dense(m->md), n, nullptr, (half_t*)output, (const half_t*)params, nullptr, false, nullptr, (const half_t*)input);
	TCNN_API_END
}

int tcnn_module_forward_half_input(tcnn_module_t* m, tcnn_stream_t stream, uint32_t n, const void* input, void* output, void* params, int prepare_input_gradients,
                                   tcnn_context_t** ctx) {
	TCNN_API_BEGIN
	if (!m || !ctx) throw std::runtime_error("tcnn_module_forward_half_input: null argument");
	if (const int r = refuse_half_input(m->md)) return r;
	auto c = std::make_unique<tcnn_context>();
	model_forward((hipStream_t)stream, nullptr, m->md, IoLayout::dense(m->md), n, nullptr, (half_t*)output, (const half_t*)params, &c->ctx, prepare_input_gradients != 0, nullptr,
	              (const half_t*)input);
	*ctx = c.release();
	TCNN_API_END
}

int tcnn_module_backward_half_input(tcnn_module_t* m, tcnn_stream_t stream, const tcnn_context_t* ctx, uint32_t n, void* dL_dinput, const void* dL_doutput, void* dL_dparams,
                                    const void* input, const void* output, const void* params) {
	(void)input;  // (the identity's backward pass does not read it)
	TCNN_API_BEGIN
	if (!m) throw std::runtime_error("tcnn_module_backward_half_input: null module");
	if (const int r = refuse_half_input(m->md)) return r;
	if (!ctx) throw std::runtime_error("backward: missing forward context");
	if (!ctx->ctx.half_input) throw std::runtime_error("backward_half_input: this context was made by tcnn_module_forward; its backward pass is tcnn_module_backward");
	model_backward((hipStream_t)stream, nullptr, m->md, IoLayout::dense(m->md), ctx->ctx, n, nullptr, (const half_t*)dL_doutput, (half_t*)dL_dparams, nullptr, (const half_t*)output,
	               (const half_t*)params, dL_dparams ? TCNN_GRADIENT_OVERWRITE : TCNN_GRADIENT_IGNORE, m->lds_level_budget, (half_t*)dL_dinput);
	TCNN_API_END
}

// cpp_api.cu:117-135 -> DifferentiableObject::backward_backward_input, implemented by the grid encoding only in the
// reference (grid.h:910-1042; object.h:468 throws for everything else).  Beyond the reference: the fp32 networks of
// tcnn_create_network_precision (model_exec.h model_backward_backward_f32), the double backward through the MLP that eikonal and
// curvature losses on a network need.
int tcnn_module_backward_backward_input(tcnn_module_t* m, tcnn_stream_t stream_, const tcnn_context_t* ctx, uint32_t n, const float* dL_ddLdinput,
                                        const float* input, const void* dL_doutput, void* dL_dparams, void* dL_ddLdoutput, float* dL_dinput,
                                        const void* params) {
	if (m->fp32_network() && fp32_second_order_network(m->md)) {
		TCNN_API_BEGIN
		if (!ctx) throw std::runtime_error("backward_backward_input: missing forward context");
		model_backward_backward_f32((hipStream_t)stream_, m->md, IoLayout::dense(m->md), ctx->ctx, n, dL_ddLdinput, (const float*)dL_doutput, (float*)dL_dparams, (float*)dL_ddLdoutput,
		                            dL_dinput, (const float*)params);
		TCNN_API_END
	}
	if (m->fp32_network() && m->md.enc.is_grid()) {  // same refusal, and what gives the same result today
		set_last_error("DifferentiableObject::backward_backward_input_impl: not implemented error: the second-order pass of an fp32 network takes the plain Identity encoding "
		               "(tcnn_create_network_precision); Encoding and Network composed in torch give the same result");
		return TCNN_ERROR_UNSUPPORTED;
	}
	if (m->md.has_network || !m->md.enc.is_grid()) {
		set_last_error("DifferentiableObject::backward_backward_input_impl: not implemented error");  // object.h:478
		return TCNN_ERROR_UNSUPPORTED;
	}
	TCNN_API_BEGIN
	if (!ctx) throw std::runtime_error("backward_backward_input: missing forward context");
	check_batch(n, widest_matrix(m->md));
	if (n == 0) return TCNN_OK;
	if (ctx->ctx.n != n) throw std::runtime_error("backward_backward_input: batch size does not match the forward context");
	if (!dL_ddLdinput) throw std::runtime_error("backward_backward_input: dL_ddLdinput is required");
	hipStream_t stream = (hipStream_t)stream_;
	const Model& md = m->md;
	const EncodingDesc& e = md.enc;
	// fp32 module with tcnn_set_fp32_second_order(1): 16-bit stand-ins for the caller's fp32 tensors (see tcnn_module::fp32_io)
	const bool fp32_kernels = m->fp32_io && g_fp32_second_order.load() == 0;
	const bool stand_ins = m->fp32_io && !fp32_kernels;
	Scratch dy16, p16, dp16, ddy16, gscale;
	void* const dL_dparams_f32 = dL_dparams;
	void* const dL_ddLdoutput_f32 = dL_ddLdoutput;
	const size_t n_out_elems = (size_t)n * e.padded_output_width;
	if (stand_ins) {
		if (dL_doutput) {
			dy16 = Fp32Bridge::gradient_to_half(stream, dL_doutput, n_out_elems, gscale);
			dL_doutput = dy16.ptr;
		}
		if (params) {
			p16 = Fp32Bridge::to_half(stream, params, md.n_params());
			params = p16.ptr;
		}
		if (dL_dparams) {
			dp16 = Scratch(stream, std::max<size_t>(md.n_params(), 1) * sizeof(half_t));
			dL_dparams = dp16.ptr;
		}
		if (dL_ddLdoutput) {
			ddy16 = Scratch(stream, std::max<size_t>(n_out_elems, 1) * sizeof(half_t));
			dL_ddLdoutput = ddy16.ptr;
		}
	}
	// the bare encoding's output is sample-major (cpp_api.cu:94-95); max_level as the forward pass of this context saw it
	GridSlice slice = grid_slice(e, IoLayout::dense(md), input, n, 1u, e.padded_output_width).max_level(ctx->ctx.max_level, ctx->ctx.max_level_gpu);
	slice.io.ddx = dL_ddLdinput;
	slice.io.ddx_stride_i = md.n_input_dims;
	slice.io.ddx_stride_d = 1u;
	const GridMeta& grid = slice.grid;
	const GridIO& io = slice.io;
	if (fp32_kernels) {  // the caller's fp32 tensors as they are: no stand-ins, no gradient scale, no 16-bit scratch
		if (dL_ddLdoutput) {  // grid.h:1012-1035
			if (!ctx->ctx.dy_dx.ptr) throw std::runtime_error("backward_backward_input: the forward pass did not prepare input gradients");
			grid_backward_backward_dLdoutput(stream, md.n_input_dims, e.n_output_dims, e.padded_output_width - e.n_output_dims, io, ctx->ctx.dy_dx.as<float>(),
			                                 (float*)dL_ddLdoutput);
		}
		if ((dL_dparams || dL_dinput) && !dL_doutput) throw std::runtime_error("backward_backward_input: dL_doutput is required for parameter / input gradients");
		if (dL_dparams && e.n_params > 0) grid_backward(stream, grid, io, (const float*)dL_doutput, (float*)dL_dparams, false);  // grid.h:942-975, GradientMode::Overwrite
		if (dL_dinput) {  // grid.h:977-1010
			if (!params) throw std::runtime_error("backward_backward_input: params are required for the input gradient");
			grid_backward_backward_input(stream, grid, io, (const float*)dL_doutput, (const float*)params, dL_dinput, md.n_input_dims, 1u);
		}
		return TCNN_OK;
	}
	if (dL_ddLdoutput) {  // grid.h:1012-1035
		if (!ctx->ctx.dy_dx.ptr) throw std::runtime_error("backward_backward_input: the forward pass did not prepare input gradients");
		grid_backward_backward_dLdoutput(stream, md.n_input_dims, e.n_output_dims, e.padded_output_width - e.n_output_dims, io, ctx->ctx.dy_dx.as<float>(),
		                                 (half_t*)dL_ddLdoutput);
	}
	if (dL_dparams || dL_dinput) {
		if (!dL_doutput) throw std::runtime_error("backward_backward_input: dL_doutput is required for parameter / input gradients");
	}
	if (dL_dparams && e.n_params > 0) {  // grid.h:942-975, GradientMode::Overwrite
		grid_backward_with_workspace(stream, slice, (const half_t*)dL_doutput, (half_t*)dL_dparams, false, GridBackwardMode::Bucketed, m->lds_level_budget);
	}
	if (dL_dinput) {  // grid.h:977-1010
		grid_backward_backward_input(stream, grid, io, (const half_t*)dL_doutput, (const half_t*)params, dL_dinput, md.n_input_dims, 1u);
	}
	if (stand_ins) {  // dL_ddLdoutput does not depend on dL_doutput; the other two carry its scale
		if (dL_ddLdoutput_f32) cast_f16_to_f32(stream, n_out_elems, ddy16.as<half_t>(), (float*)dL_ddLdoutput_f32);
		if (dL_dparams_f32) {
			if (gscale.ptr) cast_scaled_f16_to_f32(stream, md.n_params(), dp16.as<half_t>(), (float*)dL_dparams_f32, (const float*)(gscale.as<float>() + 1));
			else cast_f16_to_f32(stream, md.n_params(), dp16.as<half_t>(), (float*)dL_dparams_f32);
		}
		if (dL_dinput && gscale.ptr) scale_f32(stream, (size_t)n * md.n_input_dims, dL_dinput, (const float*)(gscale.as<float>() + 1));
	}
	TCNN_API_END
}
void tcnn_context_destroy(tcnn_context_t* ctx) { delete ctx; }

uint32_t tcnn_module_n_input_dims(const tcnn_module_t* m) { return m->md.n_input_dims; }
uint32_t tcnn_module_n_output_dims(const tcnn_module_t* m) { return m->md.padded_output_width(); }
size_t tcnn_module_n_params(const tcnn_module_t* m) { return m->md.n_params(); }
// the weight matrices that lead the module's parameter vector, in order (Optimizer::allocate's layer_sizes, object.h layer_sizes()): rows x
// cols of each into rows[] / cols[] (`capacity` entries each, may be NULL with capacity 0), their number into *n_layers.  A bare encoding has none.
int tcnn_module_network_layers(const tcnn_module_t* m, uint32_t* rows, uint32_t* cols, size_t capacity, size_t* n_layers) {
	TCNN_API_BEGIN
	std::vector<std::pair<uint32_t, uint32_t>> layers;
	if (m->md.has_network) {
		const MlpMeta& mlp = m->md.net.mlp;
		layers.emplace_back(mlp.width, mlp.in_width);
		for (uint32_t l = 0; l < mlp.n_hidden_matmuls; ++l) layers.emplace_back(mlp.width, mlp.width);
		layers.emplace_back(mlp.padded_out, mlp.width);
	}
	if (n_layers) *n_layers = layers.size();
	if (capacity && (!rows || !cols)) throw std::runtime_error("tcnn_module_network_layers: missing output array");
	for (size_t l = 0; l < layers.size() && l < capacity; ++l) {
		rows[l] = layers[l].first;
		cols[l] = layers[l].second;
	}
	TCNN_API_END
}
int tcnn_module_param_precision(const tcnn_module_t* m) { return m->fp32_io ? TCNN_PRECISION_FP32 : NATIVE_PRECISION; }
int tcnn_module_output_precision(const tcnn_module_t* m) { return m->fp32_io ? TCNN_PRECISION_FP32 : NATIVE_PRECISION; }

int tcnn_module_initialize_params(tcnn_module_t* m, size_t seed, float* params_full_precision, float scale) {
	TCNN_API_BEGIN
	Pcg32 rng{(uint64_t)seed};  // cpp_api.cu:139-142
	m->md.initialize_params(nullptr, rng, params_full_precision, scale);
	HIP_CHECK(hipStreamSynchronize(nullptr));
	TCNN_API_END
}

const char* tcnn_module_hyperparams_json(const tcnn_module_t* m) { return m->md.hyper_json.c_str(); }
const char* tcnn_module_name(const tcnn_module_t* m) { return m->name.c_str(); }
int tcnn_module_jit_fusion(const tcnn_module_t*) { return 0; }
int tcnn_module_set_jit_fusion(tcnn_module_t*, int val) {
	if (val) log_message(TCNN_LOG_WARNING, "JIT fusion was requested but this build has no runtime compilation path; the statically fused kernels are used.");
	return TCNN_OK;
}

int tcnn_module_grid_indices(tcnn_module_t* m, tcnn_stream_t stream, uint32_t n, const float* input, uint32_t* indices) {
	TCNN_API_BEGIN
	if (!m->md.enc.is_grid()) throw std::runtime_error("grid_indices: module has no grid encoding");
	GridIO io = {input, m->md.n_input_dims, 1u, n, n, 1u};
	grid_indices((hipStream_t)stream, m->md.enc.grid, io, indices);
	TCNN_API_END
}
int tcnn_module_grid_level_n_params(const tcnn_module_t* m, uint32_t level, size_t* out) {
	TCNN_API_BEGIN
	if (!m->md.enc.is_grid() || level >= m->md.enc.grid.n_levels) throw std::runtime_error("grid_level_n_params: invalid level");
	*out = m->md.enc.grid.offset[level + 1] - m->md.enc.grid.offset[level];  // multi_level_interface.h level_n_params
	TCNN_API_END
}
int tcnn_module_grid_level_params_offset(const tcnn_module_t* m, uint32_t level, size_t* out) {
	TCNN_API_BEGIN
	if (!m->md.enc.is_grid() || level >= m->md.enc.grid.n_levels) throw std::runtime_error("grid_level_params_offset: invalid level");
	*out = m->md.enc.grid.offset[level];
	TCNN_API_END
}
// MultiLevelEncoding::set_max_level / max_level / set_max_level_gpu (multi_level_interface.h:101-123): run-time state of a lone grid
int tcnn_module_set_max_level(tcnn_module_t* m, float value) {
	TCNN_API_BEGIN
	if (!m) throw std::runtime_error("tcnn_module_set_max_level: null module");
	if (const int r = refuse_max_level(m->md)) return r;
	m->md.enc.grid.max_level = value;
	TCNN_API_END
}
int tcnn_module_max_level(const tcnn_module_t* m, float* out) {
	TCNN_API_BEGIN
	if (!m || !out) throw std::runtime_error("tcnn_module_max_level: null argument");
	if (const int r = refuse_max_level(m->md)) return r;
	*out = m->md.enc.grid.max_level;
	TCNN_API_END
}
int tcnn_module_set_max_level_gpu(tcnn_module_t* m, const float* device_ptr) {
	TCNN_API_BEGIN
	if (!m) throw std::runtime_error("tcnn_module_set_max_level_gpu: null module");
	if (const int r = refuse_max_level(m->md)) return r;
	m->md.enc.max_level_gpu = device_ptr;
	TCNN_API_END
}
uint32_t tcnn_module_n_nested(const tcnn_module_t* m) { return (uint32_t)m->md.enc.nested.size(); }
int tcnn_module_nested_layout(const tcnn_module_t* m, uint32_t index, uint32_t* layout, size_t* params) {
	TCNN_API_BEGIN
	if (index >= m->md.enc.nested.size()) throw std::runtime_error("nested_layout: invalid index");
	const EncodingDesc& e = m->md.enc.nested[index];
	layout[0] = e.dims_to_encode_begin;
	layout[1] = e.n_dims;
	layout[2] = e.output_row;
	layout[3] = e.padded_output_width;
	params[0] = m->md.n_mlp_params() + e.param_offset;
	params[1] = e.n_params;
	TCNN_API_END
}

}  // extern "C"

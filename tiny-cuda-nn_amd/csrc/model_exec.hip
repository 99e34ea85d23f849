// model_exec.hip -- the forward / backward / inference passes declared in model_exec.h (host code: scratch blocks, launch order, flags).
#include "model_exec.h"

#include <algorithm>

#include "half_input_kernels.h"
#include "host_common.h"
#include "switches.h"

namespace tcnn_hip {

int refuse_max_level(const Model& md) {
	const std::string why = md.max_level_refusal();
	if (why.empty()) return TCNN_OK;
	set_last_error(why);
	return TCNN_ERROR_UNSUPPORTED;
}

std::string half_input_refusal(const Model& md) {
	const EncodingDesc& e = md.enc;
	const std::string prefix = std::string("half_input: ") + e.name();
	if (md.has_network && md.net.fp32) return "half_input: an fp32 network reads fp32 inputs: 16-bit inputs go to the 16-bit modules tcnn_create_network makes";
	if (!md.has_network) return prefix + " is a bare encoding: 16-bit inputs go to the modules tcnn_create_network makes (positions need fp32)";
	if (e.kind != EncodingKind::Identity) return prefix + " in front of the network reads fp32 inputs: 16-bit inputs go to the modules tcnn_create_network makes";
	if (e.id_scale != 1.0f || e.id_offset != 0.0f) return prefix + " with a scale other than 1 or an offset other than 0 is not exact on 16-bit values";
	return "";
}
int refuse_half_input(const Model& md) {
	const std::string why = half_input_refusal(md);
	if (why.empty()) return TCNN_OK;
	set_last_error(why);
	return TCNN_ERROR_UNSUPPORTED;
}
static uint16_t half_bits(float v) { return __builtin_bit_cast(uint16_t, (half_t)v); }

void check_batch(uint32_t n, uint32_t widest) {
	if (n % BATCH_SIZE_GRANULARITY != 0) {  // object.h:170, 217, 298
		throw std::runtime_error("Batch size " + std::to_string(n) + " must be a multiple of " + std::to_string(BATCH_SIZE_GRANULARITY) + ".");
	}
	// the element-wise kernels index (sample, feature) pairs with 32 bits
	if ((uint64_t)n * widest > 0xFFFFFFFFull) {
		throw std::runtime_error("Batch size " + std::to_string(n) + " x " + std::to_string(widest) + " features exceeds 2^32 elements; split the batch.");
	}
}
// The encodings without parameters (frequency / one-blob / identity), T = the 16-bit type or float: `out` and `dL_dy` have element
// (feature k, sample i) at [k * stride_k + i * stride_i]
template <typename T>
static void parameterless_forward(hipStream_t stream, const EncodingDesc& e, const IoLayout& layout, uint32_t n, const float* input, T* out, uint32_t stride_k, uint32_t stride_i) {
	if (e.kind == EncodingKind::Frequency) {
		frequency_forward(stream, n, e.n_dims, e.n_frequencies, e.padded_output_width, input, layout.in_stride_i, layout.in_stride_d, out, stride_k, stride_i);
	} else if (e.kind == EncodingKind::TriangleWave) {
		triangle_wave_forward(stream, n, e.n_dims, e.n_frequencies, e.padded_output_width, input, layout.in_stride_i, layout.in_stride_d, out, stride_k, stride_i);
	} else if (e.kind == EncodingKind::OneBlob) {
		oneblob_forward(stream, n, e.n_dims, e.n_bins, e.padded_output_width, input, layout.in_stride_i, layout.in_stride_d, out, stride_k, stride_i);
	} else {
		identity_forward(stream, n, e.n_dims, e.padded_output_width, e.id_scale, e.id_offset, input, layout.in_stride_i, layout.in_stride_d, out, stride_k, stride_i);
	}
}
template <typename T>
static void parameterless_backward(hipStream_t stream, const EncodingDesc& e, const IoLayout& layout, uint32_t n, const float* input, const T* dL_dy, uint32_t stride_k, uint32_t stride_i,
                                   float* dL_dinput) {
	if (e.kind == EncodingKind::Frequency) {
		frequency_backward(stream, n, e.n_dims, e.n_frequencies, dL_dy, stride_k, stride_i, input, layout.in_stride_i, layout.in_stride_d, dL_dinput, layout.dx_stride_i, layout.dx_stride_d);
	} else if (e.kind == EncodingKind::TriangleWave) {
		triangle_wave_backward(stream, n, e.n_dims, e.n_frequencies, dL_dy, stride_k, stride_i, input, layout.in_stride_i, layout.in_stride_d, dL_dinput, layout.dx_stride_i, layout.dx_stride_d);
	} else if (e.kind == EncodingKind::OneBlob) {
		oneblob_backward(stream, n, e.n_dims, e.n_bins, dL_dy, stride_k, stride_i, input, layout.in_stride_i, layout.in_stride_d, dL_dinput, layout.dx_stride_i, layout.dx_stride_d);
	} else {
		identity_backward(stream, n, e.n_dims, e.id_scale, dL_dy, stride_k, stride_i, dL_dinput, layout.dx_stride_i, layout.dx_stride_d);
	}
}


// ---- Composite encoding (composite.h:215-355), T = the 16-bit type or float.  Its nested encodings without parameters are ONE launch driven
// by a table of parts (composite_kernels.h); every nested grid runs its own kernels on its slice: input dims from dims_to_encode_begin, output
// rows from output_row, parameters and gradients from param_offset.
static EncodingParts parameterless_parts(const EncodingDesc& c) {
	EncodingParts parts;
	for (const EncodingDesc& e : c.nested) {
		if (e.is_grid()) continue;
		EncodingPart p = {};
		switch (e.kind) {
			case EncodingKind::Identity: p.kind = PART_IDENTITY; break;
			case EncodingKind::OneBlob: p.kind = PART_ONEBLOB; p.param = e.n_bins; break;
			case EncodingKind::Frequency: p.kind = PART_FREQUENCY; p.param = e.n_frequencies; break;
			case EncodingKind::TriangleWave: p.kind = PART_TRIANGLE_WAVE; p.param = e.n_frequencies; break;
			default: throw std::runtime_error("CompositeEncoding: unexpected nested encoding");
		}
		p.in_row = e.dims_to_encode_begin;
		p.in_width = e.n_dims;
		p.out_row = e.output_row;
		p.padded_width = e.padded_output_width;
		p.scale = e.id_scale;
		p.offset = e.id_offset;
		parts.add(p);
	}
	return parts;
}

// ---- the steps of one grid, lone or nested.  `rows` / `dL_dy`: the pass's matrix from the grid's first row (output_row) on.
// forward; the padded features behind the grid's own are zero (grid.h:757-766)
template <typename T>
static void grid_forward_padded(hipStream_t stream, const EncodingDesc& g, const GridSlice& s, const T* params, T* rows, float* dy_dx) {
	grid_forward(stream, s.grid, s.io, params, rows, dy_dx);
	const uint32_t n_to_pad = g.padded_output_width - g.n_output_dims;
	if (n_to_pad == 0) return;
	if (s.io.stride_k == 1u) {  // sample-major: n_to_pad columns of every sample's row
		HIP_CHECK(hipMemset2DAsync(rows + g.n_output_dims, (size_t)s.io.stride_i * sizeof(T), 0, (size_t)n_to_pad * sizeof(T), s.io.n, stream));
	} else {  // feature-major: n_to_pad whole rows
		HIP_CHECK(hipMemsetAsync(rows + (size_t)g.n_output_dims * s.io.stride_k, 0, (size_t)n_to_pad * s.io.stride_k * sizeof(T), stream));
	}
}
// the fp32 dy_dx of one grid for a pass that prepares input gradients ([(k * n + i) * D + d], grid.h:783-785), kept in `slot`
static float* take_dy_dx(hipStream_t stream, const EncodingDesc& g, uint32_t n, Scratch& slot) {
	slot = Scratch(stream, (size_t)g.n_output_dims * n * g.n_dims * sizeof(float));
	return slot.as<float>();
}
template <typename T>
static void grid_input_gradients(hipStream_t stream, const EncodingDesc& g, const IoLayout& layout, const GridSlice& s, const T* dL_dy, const Scratch& dy_dx, float* dL_dinput) {
	if (!dy_dx.ptr) throw std::runtime_error("backward: dL_dinput requested but forward was not run with prepare_input_gradients");
	grid_backward_input(stream, g.n_dims, g.n_output_dims, s.io, dL_dy, (const float*)dy_dx.ptr, dL_dinput + (size_t)g.dims_to_encode_begin * layout.dx_stride_d, layout.dx_stride_i,
	                    layout.dx_stride_d);
}

// out: element (feature k, sample i) at [k * stride_k + i * stride_i] with stride_i == 1 (feature-major) or stride_k == 1 (sample-major, stride_i = the padded width)
template <typename T>
static void composite_forward(hipStream_t stream, const EncodingDesc& c, const IoLayout& layout, uint32_t n, const float* input, const T* enc_params, T* out, uint32_t stride_k,
                              uint32_t stride_i, ForwardCtx* ctx, bool prepare_input_gradients) {
	if (c.nested.empty()) return;
	const bool reduce = c.reduction != ReductionType::Concatenation;
	// Sum / Product: the nested encodings write the unreduced matrix (kept in the context: the product's backward pass reads it), in the layout of `out`
	Scratch unreduced_local;
	T* target = out;
	uint32_t target_stride_i = stride_i;
	if (reduce) {
		Scratch& u = ctx ? ctx->unreduced : unreduced_local;
		u = Scratch(stream, (size_t)c.unreduced_width() * n * sizeof(T));
		target = u.as<T>();
		if (stride_k == 1u) target_stride_i = c.unreduced_width();
	}
	encoding_parts_forward(stream, parameterless_parts(c), n, input, layout.in_stride_i, layout.in_stride_d, target, stride_k, target_stride_i);
	if (ctx && prepare_input_gradients && c.has_nested_grid()) {
		ctx->nested_dy_dx.clear();
		ctx->nested_dy_dx.resize(c.nested.size());
	}
	for (size_t idx = 0; idx < c.nested.size(); ++idx) {
		const EncodingDesc& e = c.nested[idx];
		if (!e.is_grid()) continue;
		float* dy_dx = ctx && prepare_input_gradients ? take_dy_dx(stream, e, n, ctx->nested_dy_dx[idx]) : nullptr;
		grid_forward_padded(stream, e, grid_slice(e, layout, input, n, stride_k, target_stride_i), enc_params + e.param_offset, target + (size_t)e.output_row * stride_k, dy_dx);
	}
	if (reduce) reduce_forward(stream, c.reduction == ReductionType::Product, n, c.padded_output_width, (uint32_t)c.nested.size(), (const T*)target, stride_k, target_stride_i, out, stride_k, stride_i);
}

// dL_dinput (when asked for) of the composite; returns the gradient w.r.t. the unreduced matrix and its sample stride for the nested grids' parameter gradients
template <typename T>
static const T* composite_backward_input(hipStream_t stream, const EncodingDesc& c, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, uint32_t n_input_dims, float* dL_dinput,
                                         const T* dL_denc, uint32_t stride_k, uint32_t& stride_i, const float* input, Scratch& dL_dunreduced) {
	if (c.nested.empty()) return dL_denc;
	if (c.reduction != ReductionType::Concatenation) {  // composite.h:302-325
		const bool product = c.reduction == ReductionType::Product;
		if (product && !ctx.unreduced.ptr) throw std::runtime_error("backward: the forward context holds no unreduced matrix for the product reduction");
		const uint32_t unreduced_stride_i = stride_k == 1u ? c.unreduced_width() : stride_i;
		dL_dunreduced = Scratch(stream, (size_t)c.unreduced_width() * n * sizeof(T));
		reduce_backward(stream, product, n, c.padded_output_width, (uint32_t)c.nested.size(), (const T*)ctx.unreduced.ptr, dL_dunreduced.as<T>(), stride_k, unreduced_stride_i, dL_denc,
		                stride_k, stride_i);
		dL_denc = dL_dunreduced.as<T>();
		stride_i = unreduced_stride_i;
	}
	if (dL_dinput) {
		// one launch writes every dim: the parts' gradients, zero where no nested encoding without parameters reads; the grids overwrite theirs
		encoding_parts_backward(stream, parameterless_parts(c), n, n_input_dims, dL_denc, stride_k, stride_i, input, layout.in_stride_i, layout.in_stride_d, dL_dinput,
		                        layout.dx_stride_i, layout.dx_stride_d);
		for (size_t idx = 0; idx < c.nested.size(); ++idx) {
			const EncodingDesc& e = c.nested[idx];
			if (!e.is_grid()) continue;
			if (idx >= ctx.nested_dy_dx.size()) throw std::runtime_error("backward: dL_dinput requested but forward was not run with prepare_input_gradients");
			grid_input_gradients(stream, e, layout, grid_slice(e, layout, input, n, stride_k, stride_i), dL_denc + (size_t)e.output_row * stride_k, ctx.nested_dy_dx[idx], dL_dinput);
		}
	}
	return dL_denc;
}

bool begin_pass(hipStream_t stream, const Model& md, uint32_t n, ForwardCtx* ctx) {
	check_batch(n, widest_matrix(md));
	if (n == 0) return false;
	if (ctx) {
		ctx->stream = stream;
		ctx->n = n;
		ctx->keep_max_level(md.enc);
	}
	return true;
}

template <typename T>
void encoding_forward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const T* enc_params, T* out,
                      uint32_t stride_k, uint32_t stride_i, ForwardCtx* ctx, bool prepare_input_gradients) {
	const EncodingDesc& e = md.enc;
	ProfScope prof(profiler, stream, STAGE_GRID_FWD);
	if (e.is_composite()) {
		composite_forward(stream, e, layout, n, input, enc_params, out, stride_k, stride_i, ctx, prepare_input_gradients);
	} else if (e.is_grid()) {
		float* dy_dx = ctx && prepare_input_gradients ? take_dy_dx(stream, e, n, ctx->dy_dx) : nullptr;
		grid_forward_padded(stream, e, grid_slice(e, layout, input, n, stride_k, stride_i).max_level(e.grid.max_level, e.max_level_gpu), enc_params, out, dy_dx);
	} else {
		parameterless_forward(stream, e, layout, n, input, out, stride_k, stride_i);
	}
}
TCNN_INSTANTIATE_VALUE_TYPES(encoding_forward)

// (mlp_train_supported is false for every mlp_layer_by_layer() network: those always save their activations)
static bool backward_recomputes(const Model& md) { return g_fused_network_passes.load() != 0 && md.has_network && mlp_train_supported(md.net.mlp); }

// NetworkWithInputEncoding::forward_impl / inference_mixed_precision_impl (:60-81).  ctx == nullptr: inference.
void model_forward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, uint32_t n, const float* input, half_t* output, const half_t* params,
                          ForwardCtx* ctx, bool prepare_input_gradients, const MlpF32Output* f32, const half_t* input16) {
	if (input16 && !half_input_refusal(md).empty()) throw std::runtime_error(half_input_refusal(md));
	if (ctx) ctx->half_input = input16 != nullptr;
	if (!begin_pass(stream, md, n, ctx)) return;
	if (!md.has_network) {  // the bare encoding's output is sample-major (cpp_api.cu:94-95)
		encoding_forward(stream, profiler, md, layout, n, input, params, output, 1u, md.enc.padded_output_width, ctx, prepare_input_gradients);
		return;
	}
	// inference into the caller's fp32 matrix with an Identity encoding that pads nothing: the inference kernel reads the fp32 input itself
	// (MlpF32Input; no encoding kernel, no encoded matrix)
	const EncodingDesc& e = md.enc;
	if (!ctx && !input16 && e.kind == EncodingKind::Identity && e.n_dims == e.padded_output_width && layout.in_stride_i == e.n_dims && layout.in_stride_d == 1u &&
	    ((uintptr_t)input & 15u) == 0u && g_fused_identity_input.load() != 0 && mlp_infer_f32_input_supported(md.net.mlp, n)) {
		MlpF32Input f32_input;
		f32_input.x = input;
		f32_input.scale = e.id_scale;
		f32_input.offset = e.id_offset;
		ProfScope prof(profiler, stream, STAGE_MLP_FWD);
		// into the caller's fp32 matrix (network->inference) or into the padded 16-bit matrix (a module's inference, cpp_api.h:97)
		mlp_infer_wave(stream, md.net.mlp, n, params, nullptr, f32 ? nullptr : output, f32 ? *f32 : MlpF32Output(), &f32_input);
		return;
	}
	Scratch enc_local;
	Scratch& enc = ctx ? ctx->enc : enc_local;
	enc = Scratch(stream, (size_t)md.enc.padded_output_width * n * sizeof(half_t));
	if (input16) {  // the Identity encoding's bits (scale 1, offset 0, padding 1) without the fp32 matrix in between
		ProfScope prof_enc(profiler, stream, STAGE_GRID_FWD);
		half_input_pad(stream, n, e.n_dims, e.padded_output_width, (const uint16_t*)input16, (uint16_t*)enc.ptr, half_bits(1.0f));
	} else {
		encoding_forward(stream, profiler, md, layout, n, input, params + md.n_mlp_params(), enc.as<half_t>(), n, 1u, ctx, prepare_input_gradients);
	}
	half_t* hidden = nullptr;
	if (ctx && !backward_recomputes(md)) {
		ctx->hidden = Scratch(stream, mlp_saved_activation_bytes(md.net.mlp, n));
		hidden = ctx->hidden.as<half_t>();
	}
	ProfScope prof(profiler, stream, STAGE_MLP_FWD);
	if (f32) {  // (inference_to_f32 below checked that a kernel that stores fp32 itself takes this network)
		mlp_forward_f32(stream, md.net.mlp, n, params, enc.as<half_t>(), *f32);
		return;
	}
	mlp_forward(stream, md.net.mlp, n, params, enc.as<half_t>(), hidden, output);
}

// network->inference into the caller's fp32 matrix (object.h:214-271).  Where the register-resident inference kernel or the layer-by-layer
// network runs it, the kernel writes the fp32 elements itself; otherwise the padded 16-bit result goes through trim_and_cast as in the reference.
void inference_to_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, const half_t* params, float* out, uint32_t stride_i, uint32_t stride_j) {
	const uint32_t padded = md.padded_output_width(), width = md.output_width();
	if (md.has_network && n > 0 && mlp_forward_f32_supported(md.net.mlp, n)) {
		const MlpF32Output f32 = {out, width, stride_i, stride_j};
		model_forward(stream, nullptr, md, layout, n, input, nullptr, params, nullptr, false, &f32);
		return;
	}
	Scratch tmp(stream, (size_t)padded * n * sizeof(half_t));  // object.h:260
	model_forward(stream, nullptr, md, layout, n, input, tmp.as<half_t>(), params, nullptr, false);
	trim_and_cast(stream, n, padded, width, tmp.as<half_t>(), out, stride_i, stride_j);  // object.h:269-270
}

uint32_t widest_matrix(const Model& md) {
	uint32_t w = std::max(md.enc.padded_output_width, md.n_input_dims);
	// (the saved stack of one sample, in elements: twice the hidden layers where the pre-activations are kept)
	if (md.has_network) w = std::max(w, std::max((uint32_t)(mlp_saved_activation_bytes(md.net.mlp, 1u) / sizeof(half_t)), md.net.mlp.padded_out));
	if (md.enc.is_grid()) w = std::max(w, md.enc.n_output_dims * md.n_input_dims);  // dy_dx
	w = std::max(w, md.enc.unreduced_width());  // a Composite's Sum / Product
	for (const EncodingDesc& e : md.enc.nested) {
		if (e.is_grid()) w = std::max(w, e.n_output_dims * e.n_dims);  // a nested grid's dy_dx
	}
	return w;
}

bool begin_backward(const Model& md, const ForwardCtx& ctx, uint32_t n) {
	if (!begin_pass(nullptr, md, n)) return false;
	if (ctx.n != n) throw std::runtime_error("backward: batch size does not match the forward context");
	return true;
}

// NetworkWithInputEncoding::backward_impl (:83-113) / GridEncodingTemplated::backward_impl (grid.h:817-908)
void model_backward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const half_t* dL_doutput,
                           half_t* dL_dparams, const float* input, const half_t* output, const half_t* params, int gradient_mode,
                           uint32_t lds_level_budget, half_t* dL_dinput16) {
	if (!begin_backward(md, ctx, n)) return;
	if (dL_dinput16 && (dL_dinput || !ctx.half_input)) throw std::runtime_error("backward: a 16-bit dL_dinput belongs to a context made with a 16-bit input");
	const bool recompute = md.has_network && !ctx.hidden.ptr;  // the context holds the encoded input only (see g_fused_network_passes)
	if (recompute && (!ctx.enc.ptr || !mlp_train_supported(md.net.mlp))) {
		throw std::runtime_error("backward: this context holds no saved activations and the network has no single-kernel backward pass");
	}
	const bool want_grads = gradient_mode != TCNN_GRADIENT_IGNORE && dL_dparams != nullptr;
	const bool accumulate = gradient_mode == TCNN_GRADIENT_ACCUMULATE;
	const EncodingDesc& e = md.enc;
	if (!want_grads && !dL_dinput && !dL_dinput16) return;
	// the encoding's share of the pass, from the feature-major dL/d(encoded input) the network kernels wrote
	auto encoding_share = [&](const half_t* dL_denc, uint32_t stride_k, uint32_t stride_i) {
		if (ctx.half_input) {  // identity.h:83 with scale 1, without the fp32 matrix in between: the first n_dims rows as they are
			if (dL_dinput16) half_input_unpad(stream, n, e.n_dims, (const uint16_t*)dL_denc, (uint16_t*)dL_dinput16);
			return;
		}
		encoding_backward(stream, profiler, md, layout, ctx, n, dL_dinput, dL_denc, stride_k, stride_i, dL_dparams, want_grads, accumulate, input, lds_level_budget);
	};

	const half_t* dL_denc = dL_doutput;  // bare encoding: gradient of the encoding output, sample-major
	uint32_t stride_k = 1u, stride_i = e.padded_output_width;
	Scratch denc;
	if (md.has_network) {
		const bool need_denc = (want_grads && e.n_params > 0) || dL_dinput || dL_dinput16;
		ProfScope prof(profiler, stream, STAGE_MLP_BWD);
		Scratch params_t(stream, md.n_mlp_params() * sizeof(half_t));
		mlp_transpose_weights(stream, md.net.mlp, params, params_t.as<half_t>());
		const uint32_t n_partials = recompute ? mlp_train_n_partials(md.net.mlp, n, LossType::L2) : mlp_backward_n_partials(md.net.mlp, n);
		Scratch partials;
		if (want_grads) partials = Scratch(stream, (size_t)n_partials * md.n_mlp_params() * sizeof(float));
		if (need_denc) denc = Scratch(stream, (size_t)e.padded_output_width * n * sizeof(half_t));
		if (recompute) {  // forward from the encoded input again, then backward from the caller's dL/doutput, in one kernel
			MlpLossArgs la = {LossType::L2, nullptr, nullptr, md.output_width(), 1.0f, 1u};
			la.external_dL_doutput = dL_doutput;
			const SlabOrder order = mlp_train(stream, md.net.mlp, n, params, params_t.as<half_t>(), ctx.enc.as<half_t>(), la, nullptr, nullptr,
			                                  need_denc ? denc.as<half_t>() : nullptr, want_grads ? partials.as<float>() : nullptr, nullptr);
			if (want_grads) mlp_finalize_gradients(stream, md.net.mlp, n_partials, partials.as<float>(), dL_dparams, accumulate, order);
			if (!need_denc) return;
			dL_denc = denc.as<half_t>();
			stride_k = n;
			stride_i = 1u;
			encoding_share(dL_denc, stride_k, stride_i);
			return;
		}
		Scratch dpre;  // output activation: continue from dL/d(pre-activation) (fully_fused_mlp.cu:760-763)
		if (md.net.mlp.output_activation != (uint32_t)Activation::None) {
			if (!output) throw std::runtime_error("backward: the network output is required when an output activation is set");
			dpre = Scratch(stream, (size_t)md.padded_output_width() * n * sizeof(half_t));
			mlp_output_activation_backward(stream, md.net.mlp, n, output, dL_doutput, dpre.as<half_t>());
			dL_doutput = dpre.as<half_t>();
		}
		Scratch deep;
		if (const size_t deep_bytes = mlp_backward_workspace_bytes(md.net.mlp, n)) deep = Scratch(stream, deep_bytes);
		mlp_backward(stream, md.net.mlp, n, params_t.as<half_t>(), ctx.enc.as<half_t>(), ctx.hidden.as<half_t>(), dL_doutput,
		             need_denc ? denc.as<half_t>() : nullptr, want_grads ? partials.as<float>() : nullptr, deep.ptr);
		if (want_grads) mlp_finalize_gradients(stream, md.net.mlp, n_partials, partials.as<float>(), dL_dparams, accumulate);
		if (!need_denc) return;
		dL_denc = denc.as<half_t>();
		stride_k = n;
		stride_i = 1u;
	}

	encoding_share(dL_denc, stride_k, stride_i);
}

// ---- the fp32 network (mlp_kernels.h mlp_f32_*) behind the encoding's fp32 path --------------------------------------------------------------
void model_forward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, uint32_t n, const float* input, float* output, const float* params, ForwardCtx* ctx,
                       bool prepare_input_gradients, const MlpF32Output* trimmed) {
	if (!md.has_network || !md.net.fp32) throw std::runtime_error("model_forward_f32: not an fp32 network");
	if (trimmed && ctx) throw std::runtime_error("model_forward_f32: the trimmed output is for inference");
	if (ctx) ctx->half_input = false;
	if (!begin_pass(stream, md, n, ctx)) return;
	Scratch enc_local;
	Scratch& enc = ctx ? ctx->enc : enc_local;
	enc = Scratch(stream, (size_t)md.enc.padded_output_width * n * sizeof(float));
	encoding_forward(stream, nullptr, md, layout, n, input, params + md.n_mlp_params(), enc.as<float>(), n, 1u, ctx, prepare_input_gradients);
	float* hidden = nullptr;
	if (ctx) {
		ctx->hidden = Scratch(stream, mlp_f32_saved_activation_bytes(md.net.mlp, n));
		hidden = ctx->hidden.as<float>();
	}
	mlp_f32_forward(stream, md.net.mlp, n, params, enc.as<float>(), hidden, trimmed ? nullptr : output, trimmed ? *trimmed : MlpF32Output());
}

void model_backward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const float* dL_doutput, float* dL_dparams,
                        const float* input, const float* output, const float* params, int gradient_mode) {
	if (!md.has_network || !md.net.fp32) throw std::runtime_error("model_backward_f32: not an fp32 network");
	if (!begin_backward(md, ctx, n)) return;
	if (!ctx.enc.ptr || !ctx.hidden.ptr) throw std::runtime_error("backward: this context holds no saved activations of an fp32 network");
	const bool want_grads = gradient_mode != TCNN_GRADIENT_IGNORE && dL_dparams != nullptr;
	const bool accumulate = gradient_mode == TCNN_GRADIENT_ACCUMULATE;
	if (!want_grads && !dL_dinput) return;
	const EncodingDesc& e = md.enc;
	const MlpMeta& mlp = md.net.mlp;
	const bool need_denc = (want_grads && e.n_params > 0) || dL_dinput;
	Scratch params_t(stream, md.n_mlp_params() * sizeof(float));
	mlp_f32_transpose_weights(stream, mlp, params, params_t.as<float>());
	const uint32_t n_partials = mlp_f32_n_partials(mlp, n);
	Scratch partials, denc, dpre;
	if (want_grads) partials = Scratch(stream, (size_t)n_partials * md.n_mlp_params() * sizeof(float));
	if (need_denc) denc = Scratch(stream, (size_t)e.padded_output_width * n * sizeof(float));
	if (mlp.output_activation != (uint32_t)Activation::None) {  // continue from dL/d(pre-activation) (fully_fused_mlp.cu:760-763)
		if (!output) throw std::runtime_error("backward: the network output is required when an output activation is set");
		dpre = Scratch(stream, (size_t)mlp.padded_out * n * sizeof(float));
		mlp_f32_output_activation_backward(stream, mlp, n, output, dL_doutput, dpre.as<float>());
		dL_doutput = dpre.as<float>();
	}
	Scratch workspace(stream, mlp_f32_backward_workspace_bytes(mlp, n));
	mlp_f32_backward(stream, mlp, n, params_t.as<float>(), ctx.enc.as<float>(), ctx.hidden.as<float>(), dL_doutput, need_denc ? denc.as<float>() : nullptr,
	                 want_grads ? partials.as<float>() : nullptr, workspace.ptr);
	if (want_grads) mlp_f32_finalize_gradients(stream, mlp, n_partials, partials.as<float>(), dL_dparams, accumulate);
	if (need_denc) encoding_backward(stream, nullptr, md, layout, ctx, n, dL_dinput, (const float*)denc.as<float>(), n, 1u, dL_dparams, want_grads, accumulate, input);
}

bool fp32_second_order_network(const Model& md) {
	const EncodingDesc& e = md.enc;
	return md.has_network && md.net.fp32 && e.kind == EncodingKind::Identity && e.id_scale == 1.0f && e.id_offset == 0.0f;
}

// The second-order pass of an fp32 network behind the plain Identity encoding (fp32_second_order_network): mlp_f32_backward_backward between
// the encoding's two linear steps -- v = dL_ddLdinput padded with zeros into the network's feature-major input layout, and the network's
// dL/d(encoded input) trimmed back to the caller's [n][n_input_dims].  dL_dparams is overwritten, as by tcnn_module_backward.
void model_backward_backward_f32(hipStream_t stream, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, const float* dL_ddLdinput, const float* dL_doutput,
                                 float* dL_dparams, float* dL_ddLdoutput, float* dL_dinput, const float* params) {
	if (!fp32_second_order_network(md)) throw std::runtime_error("model_backward_backward_f32: not an fp32 network behind the plain Identity encoding");
	check_batch(n, widest_matrix(md));
	if (n == 0) return;
	if (ctx.n != n) throw std::runtime_error("backward_backward_input: batch size does not match the forward context");
	if (!dL_ddLdinput) throw std::runtime_error("backward_backward_input: dL_ddLdinput is required");
	if (!ctx.enc.ptr || !ctx.hidden.ptr) throw std::runtime_error("backward_backward_input: this context holds no saved activations of an fp32 network");
	if (!dL_dparams && !dL_ddLdoutput && !dL_dinput) return;
	if ((dL_dparams || dL_dinput) && !dL_doutput) throw std::runtime_error("backward_backward_input: dL_doutput is required for parameter / input gradients");
	if (!params) throw std::runtime_error("backward_backward_input: params are required");
	const EncodingDesc& e = md.enc;
	const MlpMeta& mlp = md.net.mlp;
	const uint32_t IN = e.padded_output_width;
	const bool transposed = dL_dparams || (dL_dinput && mlp_f32_second_order_has_curvature(mlp));
	Scratch v(stream, (size_t)IN * n * sizeof(float));
	identity_forward(stream, n, e.n_dims, e.n_dims, 1.0f, 0.0f, dL_ddLdinput, md.n_input_dims, 1u, v.as<float>(), n, 1u);
	if (IN > e.n_dims) HIP_CHECK(hipMemsetAsync(v.as<float>() + (size_t)e.n_dims * n, 0, (size_t)(IN - e.n_dims) * n * sizeof(float), stream));
	Scratch params_t, partials, denc;
	if (transposed) {
		params_t = Scratch(stream, md.n_mlp_params() * sizeof(float));
		mlp_f32_transpose_weights(stream, mlp, params, params_t.as<float>());
	}
	const uint32_t n_partials = mlp_f32_n_partials(mlp, n);
	if (dL_dparams) partials = Scratch(stream, (size_t)n_partials * md.n_mlp_params() * sizeof(float));
	if (dL_dinput) denc = Scratch(stream, (size_t)IN * n * sizeof(float));
	Scratch workspace(stream, mlp_f32_backward_backward_workspace_bytes(mlp, n));
	mlp_f32_backward_backward(stream, mlp, n, params, transposed ? params_t.as<float>() : nullptr, ctx.enc.as<float>(), ctx.hidden.as<float>(), v.as<float>(), dL_doutput, dL_ddLdoutput,
	                          dL_dinput ? denc.as<float>() : nullptr, dL_dparams ? partials.as<float>() : nullptr, workspace.ptr);
	if (dL_dparams) mlp_f32_finalize_gradients(stream, mlp, n_partials, partials.as<float>(), dL_dparams, false);
	if (dL_dinput) identity_backward(stream, n, e.n_dims, 1.0f, (const float*)denc.as<float>(), n, 1u, dL_dinput, layout.dx_stride_i, layout.dx_stride_d);
}

static void grid_backward_phase_hook(void* user, int phase, int begin) {
	PhaseTimer& t = *(PhaseTimer*)user;
	Profiler* p = t.profiler;
	const int stage = phase == 0 ? STAGE_GRID_BWD_SCATTER : STAGE_GRID_BWD;
	if (!p || (p->only_stage >= 0 && p->only_stage != stage)) return;
	if (begin) {
		t.a = p->get();
		HIP_CHECK(hipEventRecord(t.a, t.stream));
	} else if (t.a) {
		hipEvent_t b = p->get();
		HIP_CHECK(hipEventRecord(b, t.stream));
		p->spans.push_back({stage, t.a, b, t.counts});
		t.a = nullptr;
	}
}

// levels [a, b) of a grid as a grid of their own: the kernels index dL_dy and the gradients from the first of them
static GridMeta grid_levels(const GridMeta& g, uint32_t a, uint32_t b) {
	GridMeta s = g;
	s.n_levels = b - a;
	for (uint32_t l = 0; l <= b - a; ++l) s.offset[l] = g.offset[a + l] - g.offset[a];
	for (uint32_t l = 0; l < b - a; ++l) {
		s.scale[l] = g.scale[a + l];
		s.resolution[l] = g.resolution[a + l];
	}
	return s;
}

// consecutive levels in `n_groups` groups, cut where the running parameter count passes k / n_groups of the total
struct LevelRanges {
	uint32_t n = 0;
	uint32_t begin[MAX_N_LEVELS], end[MAX_N_LEVELS];
};
static LevelRanges split_levels(const GridMeta& g, uint32_t n_groups) {
	const uint32_t L = g.n_levels;
	LevelRanges ranges;
	for (uint32_t k = 1, a = 0; k <= n_groups && a < L; ++k) {
		uint32_t b = a + 1;
		const uint64_t target = (uint64_t)g.offset[L] * k / n_groups;
		while (b < L && (k == n_groups || g.offset[b] < target)) ++b;
		if (k == n_groups) b = L;
		ranges.begin[ranges.n] = a;
		ranges.end[ranges.n++] = b;
		a = b;
	}
	return ranges;
}

void grid_backward_with_workspace(hipStream_t stream, const GridSlice& s, const half_t* dL_dy, half_t* grid_gradient, bool accumulate, GridBackwardMode mode,
                                  uint32_t lds_level_budget, PhaseTimer* timer, const LevelGroups* groups, size_t first_param) {
	const GridMeta& grid = s.grid;
	const uint32_t L = grid.n_levels, F = grid.n_feat, n = s.io.n;
	// level groups: only where a level's treatment does not depend on its index among ALL levels (every level switched on,
	// no per-level random stream) and nothing else rides on the pass
	uint32_t n_groups = groups ? std::min(std::max(groups->n_groups, 1u), L) : 1u;
	if (grid.max_level < 1.0f || s.io.max_level || grid.stochastic != 0u) n_groups = 1;
	const LevelRanges ranges = split_levels(grid, n_groups);
	// one workspace for all groups: the largest any of them asks for (a group of later levels can bucket levels that the plan of
	// the whole grid, which takes the first MAX_BUCKET_LEVELS eligible ones, left to the other kinds)
	GridBackwardWorkspace ws;
	if (ranges.n <= 1) ws = grid_backward_workspace_size(grid, n, mode, lds_level_budget);
	for (uint32_t r = 0; ranges.n > 1 && r < ranges.n; ++r) {
		const GridBackwardWorkspace w = grid_backward_workspace_size(grid_levels(grid, ranges.begin[r], ranges.end[r]), n, mode, lds_level_budget);
		ws.scratch_bytes = std::max(ws.scratch_bytes, w.scratch_bytes);
		ws.n_counters = std::max(ws.n_counters, w.n_counters);
	}
	Scratch queues;
	if (ws.scratch_bytes) {
		queues = Scratch(stream, ws.scratch_bytes);
		ws.scratch = queues.ptr;
		ws.scratch_bytes = queues.bytes;
		ws.counters = ZeroedCounters::get(stream, ws.n_counters);
	}
	if (timer) {  // per-kernel timing when a profiler is attached
		ws.phase_hook = grid_backward_phase_hook;
		ws.hook_user = timer;
	}
	// Overwrite vs Accumulate (grid.h:865-867) is handled inside: the owner-computes kernel stores whole slices, so the reference's
	// full-table memset is only issued for the atomic A/B mode.
	for (uint32_t r = 0; r < std::max(ranges.n, 1u); ++r) {
		const uint32_t a = ranges.n > 1 ? ranges.begin[r] : 0u, b = ranges.n > 1 ? ranges.end[r] : L;
		grid_backward(stream, ranges.n > 1 ? grid_levels(grid, a, b) : grid, s.io, dL_dy + (size_t)a * F * s.io.stride_k, grid_gradient + (size_t)grid.offset[a] * F, accumulate, mode,
		              lds_level_budget, ws);
		if (timer) timer->counts = false;  // one backward pass per step, however many launch sequences it takes
		if (groups && groups->ready) groups->ready(groups->ctx, first_param + (size_t)grid.offset[a] * F, first_param + (size_t)grid.offset[b] * F);
	}
}

// One grid's parameter gradients in the pass's value type.  16-bit: the chosen backward mode with its LDS budget and workspace, level groups
// with the `ready` callback, the profiler's stages.  fp32: the reference's one formulation has none of them.
static void grid_parameter_gradients(hipStream_t stream, PhaseTimer& timer, const GridSlice& s, const half_t* dL_dy, half_t* grid_gradient, bool accumulate, uint32_t lds_level_budget,
                                     const LevelGroups* groups, size_t first_param) {
	grid_backward_with_workspace(stream, s, dL_dy, grid_gradient, accumulate, (GridBackwardMode)g_grid_backward_mode.load(), lds_level_budget, &timer, groups, first_param);
}
static void grid_parameter_gradients(hipStream_t stream, PhaseTimer&, const GridSlice& s, const float* dL_dy, float* grid_gradient, bool accumulate, uint32_t, const LevelGroups*, size_t) {
	grid_backward(stream, s.grid, s.io, dL_dy, grid_gradient, accumulate);
}

// The encoding's share of the backward pass, from dL/d(encoded input) -- the feature-major matrix the network kernels wrote, or a bare
// encoding's sample-major dL_doutput: dL_denc has element (feature k, sample i) at [k * stride_k + i * stride_i].
template <typename T>
void encoding_backward(hipStream_t stream, Profiler* profiler, const Model& md, const IoLayout& layout, const ForwardCtx& ctx, uint32_t n, float* dL_dinput, const T* dL_denc,
                       uint32_t stride_k, uint32_t stride_i, T* dL_dparams, bool want_grads, bool accumulate, const float* input, uint32_t lds_level_budget,
                       const LevelGroups* groups) {
	const EncodingDesc& e = md.enc;
	want_grads = want_grads && dL_dparams && e.n_params > 0;
	T* enc_grads = want_grads ? dL_dparams + md.n_mlp_params() : nullptr;
	PhaseTimer timer = {profiler, stream};
	if (e.is_composite()) {
		Scratch dL_dunreduced;
		dL_denc = composite_backward_input(stream, e, layout, ctx, n, md.n_input_dims, dL_dinput, dL_denc, stride_k, stride_i, input, dL_dunreduced);
		if (!want_grads) return;
		// every nested grid on its own slice of dL_dy, its gradients at its own parameter offset: Overwrite / Accumulate hold per slice, the
		// workspace is taken per grid (the plain path: no level groups)
		for (const EncodingDesc& g : e.nested) {
			if (!g.is_grid() || g.n_params == 0) continue;
			grid_parameter_gradients(stream, timer, grid_slice(g, layout, input, n, stride_k, stride_i), dL_denc + (size_t)g.output_row * stride_k, enc_grads + g.param_offset, accumulate,
			                         lds_level_budget, nullptr, 0);
		}
		if (groups && groups->ready) groups->ready(groups->ctx, md.n_mlp_params(), md.n_params());
	} else if (e.is_grid()) {
		// max_level as the forward pass of this context saw it
		const GridSlice s = grid_slice(e, layout, input, n, stride_k, stride_i).max_level(ctx.max_level, ctx.max_level_gpu);
		if (want_grads) grid_parameter_gradients(stream, timer, s, dL_denc, enc_grads, accumulate, lds_level_budget, groups, md.n_mlp_params());
		if (dL_dinput) grid_input_gradients(stream, e, layout, s, dL_denc, ctx.dy_dx, dL_dinput);
	} else if (dL_dinput) {
		parameterless_backward(stream, e, layout, n, input, dL_denc, stride_k, stride_i, dL_dinput);
	}
}
TCNN_INSTANTIATE_VALUE_TYPES(encoding_backward)

}  // namespace tcnn_hip

// api_optimizer.hip -- C ABI: the stand-alone optimizer (tcnn_optimizer_*) and tcnn_loss_evaluate, for hosts that drive the passes themselves.
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "device_alloc.h"
#include "host_common.h"
#include "model_desc.h"
#include "optimizer_chain.h"
#include "optimizer_kernels_f32.h"

using namespace tcnn_hip;

extern "C" {

// Optimizer<T> on its own (optimizer.h:40-99): an optimizer chain (optimizer_chain.h) over weight buffers the HOST owns -- for callers that
// drive forward / loss / backward themselves.  The same kernels and arithmetic as the trainer's optimizer step (Adam: counter form of the
// per-parameter step counters).
struct tcnn_optimizer {
	std::unique_ptr<OptimizerChain> chain;
	std::string hyper_json;
};
int tcnn_create_optimizer(const char* optimizer_json, tcnn_optimizer_t** out) {
	TCNN_API_BEGIN
	auto o = std::make_unique<tcnn_optimizer>();
	o->chain = std::make_unique<OptimizerChain>(Json::parse(optimizer_json ? optimizer_json : "{}"));
	*out = o.release();
	TCNN_API_END
}
// Optimizer<T> with T by `requested_precision`: the library's own 16-bit precision gives exactly what tcnn_create_optimizer gives;
// TCNN_PRECISION_FP32 the reference's Optimizer<float> (optimizer_kernels_f32.h): one float weight vector, float gradients, float wrapper state
int tcnn_create_optimizer_precision(const char* optimizer_json, int requested_precision, tcnn_optimizer_t** out) {
	if (requested_precision == NATIVE_PRECISION) return tcnn_create_optimizer(optimizer_json, out);
	TCNN_API_BEGIN
	if (requested_precision != TCNN_PRECISION_FP32) {
		set_last_error(HALF_IS_BF16 ? "create_optimizer: this build (libtcnn_hip_bf16.so) provides bf16 and fp32 optimizers, not fp16 ones"
		                            : "create_optimizer: this build provides fp16 and fp32 optimizers, not bf16 ones");
		return TCNN_ERROR_UNSUPPORTED;
	}
	auto o = std::make_unique<tcnn_optimizer>();
	o->chain = std::make_unique<OptimizerChain>(Json::parse(optimizer_json ? optimizer_json : "{}"), /*fp32=*/true);
	*out = o.release();
	TCNN_API_END
}
int tcnn_optimizer_precision(const tcnn_optimizer_t* o) { return o->chain->fp32() ? TCNN_PRECISION_FP32 : NATIVE_PRECISION; }
// Optimizer::allocate(n_weights, layer_sizes): the layers' weight matrices lead the parameter vector (weight decay / l2_reg of Adam apply to
// them, adam.h:79-110; Novograd steps them alone, layer by layer), the rest (e.g. an encoding's) are no matrix weights
int tcnn_optimizer_allocate_layers(tcnn_optimizer_t* o, size_t n_weights, size_t n_layers, const uint32_t* rows, const uint32_t* cols) {
	TCNN_API_BEGIN
	if (n_weights > 0xFFFFFFFFull || (n_layers && (!rows || !cols))) throw std::runtime_error("Optimizer::allocate: bad sizes");
	std::vector<std::pair<uint32_t, uint32_t>> layers;
	for (size_t l = 0; l < n_layers; ++l) layers.emplace_back(rows[l], cols[l]);
	o->chain->allocate((uint32_t)n_weights, layers);
	TCNN_API_END
}
// one layer of n_matrix_weights x 1 when n_matrix_weights > 0
int tcnn_optimizer_allocate(tcnn_optimizer_t* o, size_t n_weights, size_t n_matrix_weights) {
	if (n_matrix_weights > 0xFFFFFFFFull) n_matrix_weights = 0xFFFFFFFFull;  // (refused below: more than n_weights can hold)
	const uint32_t rows = (uint32_t)n_matrix_weights, cols = 1u;
	return tcnn_optimizer_allocate_layers(o, n_weights, n_matrix_weights > 0 ? 1 : 0, &rows, &cols);
}
// Optimizer::step (optimizer.h:58): gradients carry the loss scale; weights_full_precision and weights (16-bit) are both updated
int tcnn_optimizer_step(tcnn_optimizer_t* o, tcnn_stream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients) {
	TCNN_API_BEGIN
	if (!o->chain->n_weights()) return TCNN_OK;
	if (o->chain->fp32()) {  // one float weight vector: gradients are floats, `weights` names the same buffer or nothing
		if (!weights_full_precision || !gradients) throw std::runtime_error("Optimizer::step: missing buffer");
		if (weights && weights != (void*)weights_full_precision) {
			throw std::runtime_error("Optimizer::step: an fp32 optimizer steps ONE float weight vector: `weights` must be NULL or equal to `weights_full_precision`");
		}
		o->chain->step((hipStream_t)stream, loss_scale, weights_full_precision, nullptr, gradients);
		return TCNN_OK;
	}
	if (!weights_full_precision || !weights || !gradients) throw std::runtime_error("Optimizer::step: missing buffer");
	o->chain->step((hipStream_t)stream, loss_scale, weights_full_precision, weights, gradients);
	TCNN_API_END
}
uint32_t tcnn_optimizer_step_count(const tcnn_optimizer_t* o) { return o->chain->step_count(); }
int tcnn_optimizer_update_hyperparams(tcnn_optimizer_t* o, const char* optimizer_json) {
	TCNN_API_BEGIN
	o->chain->update_hyperparams(Json::parse(optimizer_json ? optimizer_json : "{}"));
	TCNN_API_END
}
const char* tcnn_optimizer_hyperparams_json(tcnn_optimizer_t* o) {
	o->hyper_json = o->chain->hyperparams().dump();
	return o->hyper_json.c_str();
}
// Adam's buffers: which = 0 first moments, 1 second moments (fp32), 2 per-parameter step counters (u32); device pointers, n_weights elements each
void* tcnn_optimizer_state(tcnn_optimizer_t* o, int which) {
	void* p = nullptr;
	if (o->chain->base() != OptimizerChain::Kind::Adam) {
		set_last_error("tcnn_optimizer_state: the base optimizer is not Adam (use tcnn_optimizer_state_named)");
		return nullptr;
	}
	o->chain->state_named(which == 0 ? "first_moments" : which == 1 ? "second_moments" : which == 2 ? "param_steps" : "", &p, nullptr, nullptr);
	return p;
}
// any state buffer of the chain by its snapshot key without "_binary" (weights_lookahead, weights_average, weights_samples, averaged_gradients,
// averaged_gradients_half, first_moments, per_layer_second_moments, weights_ema, ...): device pointer, element count, bytes per element
int tcnn_optimizer_state_named(tcnn_optimizer_t* o, const char* name, void** ptr, size_t* count, size_t* elem_bytes) {
	TCNN_API_BEGIN
	if (!name || !o->chain->state_named(name, ptr, count, elem_bytes)) throw std::runtime_error(std::string("Optimizer: no state buffer named '") + (name ? name : "") + "' in this optimizer");
	TCNN_API_END
}
// Optimizer::custom_weights(): the outermost wrapper's inference weights (Ema's average, Lookahead's slow weights, Average's mean), or null
void* tcnn_optimizer_custom_weights(tcnn_optimizer_t* o) { return o->chain->custom_weights(); }
// Optimizer::serialize() / deserialize(): the state as the MessagePack bytes of the reference's JSON document (snapshot_msgpack.h; the
// "optimizer" member of a trainer snapshot).  buffer == NULL: *n_bytes = the size needed.
int tcnn_optimizer_serialize(tcnn_optimizer_t* o, void* buffer, size_t capacity, size_t* n_bytes) {
	TCNN_API_BEGIN
	std::vector<uint8_t> header;
	msgpack_detail::Writer count{header, true};
	o->chain->write_state(count);
	const size_t needed = header.size() + count.skipped;
	if (n_bytes) *n_bytes = needed;
	if (buffer) {
		if (capacity < needed) throw std::runtime_error("tcnn_optimizer_serialize: buffer too small");
		HIP_CHECK(hipDeviceSynchronize());
		std::vector<uint8_t> bytes;
		bytes.reserve(needed);
		msgpack_detail::Writer w{bytes};
		o->chain->write_state(w);
		std::memcpy(buffer, bytes.data(), bytes.size());
	}
	TCNN_API_END
}
int tcnn_optimizer_deserialize(tcnn_optimizer_t* o, const void* data, size_t n_bytes) {
	TCNN_API_BEGIN
	if (!data) throw std::runtime_error("tcnn_optimizer_deserialize: null data");
	HIP_CHECK(hipDeviceSynchronize());
	msgpack_detail::Reader r{(const uint8_t*)data, (const uint8_t*)data + n_bytes};
	o->chain->read_state(r);
	HIP_CHECK(hipDeviceSynchronize());
	TCNN_API_END
}
void tcnn_optimizer_destroy(tcnn_optimizer_t* o) { delete o; }

// Loss<T>::evaluate (loss.h:42-50) on its own: prediction / gradients are column-major `stride` x n matrices in the library's 16-bit
// type (= sample-major [n][stride]), target / data_pdf `dims` x n fp32, values `stride` x n fp32 (may be null); rows >= dims carry no
// loss (relative_l2.h:57-61).  Normalised by n * dims like the reference's kernels (n_elements / stride * dims).
int tcnn_loss_evaluate(const char* loss_otype, tcnn_stream_t stream, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const void* prediction,
                       const float* target, const float* data_pdf, float* values, void* gradients) {
	TCNN_API_BEGIN
	if (!loss_otype || !prediction || !target || !gradients) throw std::runtime_error("Loss::evaluate: missing argument");
	if (stride % 8 != 0 || dims > stride) throw std::runtime_error("Loss::evaluate: the prediction's row count must be a multiple of 8 and at least the target's");
	if ((uint64_t)n * dims > 0xFFFFFFFFull || (uint64_t)n * stride > 0xFFFFFFFFull) throw std::runtime_error("Loss::evaluate: batch too large");
	if (n == 0) return TCNN_OK;
	loss_evaluate((hipStream_t)stream, string_to_loss(loss_otype), n, stride, dims, loss_scale, (const half_t*)prediction, target, data_pdf, values, (half_t*)gradients,
	              nullptr, n * dims);
	TCNN_API_END
}

// the same with prediction / gradients in `requested_precision`: the library's 16-bit one is tcnn_loss_evaluate; TCNN_PRECISION_FP32 takes
// float matrices (Loss<float>: the same arithmetic, the gradient is not rounded to 16 bits)
int tcnn_loss_evaluate_precision(const char* loss_otype, tcnn_stream_t stream, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, int requested_precision,
                                 const void* prediction, const float* target, const float* data_pdf, float* values, void* gradients) {
	if (requested_precision == NATIVE_PRECISION) return tcnn_loss_evaluate(loss_otype, stream, n, stride, dims, loss_scale, prediction, target, data_pdf, values, gradients);
	TCNN_API_BEGIN
	if (requested_precision != TCNN_PRECISION_FP32) {
		set_last_error(HALF_IS_BF16 ? "Loss::evaluate: this build (libtcnn_hip_bf16.so) provides bf16 and fp32 losses, not fp16 ones"
		                            : "Loss::evaluate: this build provides fp16 and fp32 losses, not bf16 ones");
		return TCNN_ERROR_UNSUPPORTED;
	}
	if (!loss_otype || !prediction || !target || !gradients) throw std::runtime_error("Loss::evaluate: missing argument");
	if (stride % 8 != 0 || dims > stride) throw std::runtime_error("Loss::evaluate: the prediction's row count must be a multiple of 8 and at least the target's");
	if ((uint64_t)n * dims > 0xFFFFFFFFull || (uint64_t)n * stride > 0xFFFFFFFFull) throw std::runtime_error("Loss::evaluate: batch too large");
	if (n == 0) return TCNN_OK;
	loss_evaluate_f32((hipStream_t)stream, string_to_loss(loss_otype), n, stride, dims, loss_scale, (const float*)prediction, target, data_pdf, values, (float*)gradients,
	                  n * dims);
	TCNN_API_END
}

}  // extern "C"

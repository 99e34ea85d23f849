// optimizer_chain.h -- an optimizer as the reference composes it (optimizer.cu:50-86): wrappers (Ema, ExponentialDecay, Lookahead, Average,
// Batched; any order, each at most once) around exactly one base (Adam, SGD, Novograd).  Host-side object over weight / gradient buffers
// it does not own; behind the stand-alone tcnn_optimizer and, for every chain besides the trainer's built-in Adam / Ema /
// ExponentialDecay path, behind the trainer.
// A chain is built for one value type T of weights / gradients / wrapper state: the library's 16-bit type (fp32 master weights beside the
// 16-bit ones), or float (`fp32`: the reference's Optimizer<float> -- ONE float weight vector, float gradients, float wrapper state; the
// kernels of optimizer_kernels_f32.h).  Host logic, hyperparameters and snapshot layout are the same; buffers of type T are `void*` here.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/tiny-cuda-nn/json_mini.h"
#include "elementwise_kernels.h"
#include "optimizer_kernels.h"
#include "optimizer_kernels_f32.h"
#include "snapshot_msgpack.h"

namespace tcnn_hip {

class OptimizerChain {
public:
	enum class Kind { Adam, SGD, Novograd, Ema, ExponentialDecay, Lookahead, Average, Batched };
	static const char* kind_name(Kind k);  // the reference's otype spelling (hyperparams())

	explicit OptimizerChain(const Json& config, bool fp32 = false);  // parses; touches no device
	~OptimizerChain();
	OptimizerChain(const OptimizerChain&) = delete;
	OptimizerChain& operator=(const OptimizerChain&) = delete;

	// Optimizer::allocate(n_weights, layer_sizes): the layers' rows x cols weight matrices lead the parameter vector
	void allocate(uint32_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes);
	// Optimizer::step over the whole parameter vector; everything is enqueued on `stream` (capturable)
	// (fp32 chain: `weights` is not used -- weights_full_precision IS the weight vector -- and `gradients` points to floats)
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients);
	// the same over [begin, end) of the current step; `advance`: this call opens the step (counters, schedule).  Only chains of
	// SGD / Adam / Ema / ExponentialDecay (ranged_refusal() == nullptr)
	void step_range(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, uint32_t begin, uint32_t end, bool advance);
	// which launches the NEXT step() will enqueue, as a number: the wrappers' host logic changes them from step to step (Lookahead's copy
	// and pull, Batched's nested step), and a step captured into a graph can only patch an instantiated graph of the same launches
	uint32_t next_step_signature() const;
	const char* ranged_refusal() const;  // the outermost optimizer of the chain that cannot step by parameter range, or nullptr

	uint32_t step_count() const { return step_count(0); }  // Optimizer::step(): Batched reports its own count, the other wrappers the nested one
	float learning_rate() const;
	void set_learning_rate(float v);
	void* custom_weights() const { return custom_weights(0); }  // (type T) the outermost wrapper's inference weights, nullptr if none has any
	void update_hyperparams(const Json& config);  // throws "optimizer structure does not match" when the otypes differ
	Json hyperparams() const { return hyperparams(0); }

	uint32_t n_weights() const { return m_n; }
	bool fp32() const { return m_fp32; }
	Kind base() const { return m_nodes.back().kind; }
	bool contains(Kind k) const;
	// state buffers by the snapshot keys without "_binary" (device pointers); false if the chain has none of that name
	bool state_named(const std::string& name, void** ptr, size_t* count, size_t* elem_bytes) const;

	// the state as the reference's serialize() lays it out, keys in lexicographic order (snapshot_msgpack.h); synchronises the device
	void write_state(msgpack_detail::Writer& w) const { write_state(w, 0); }
	void read_state(msgpack_detail::Reader& r) { read_state(r, 0); }

private:
	struct Node {
		Kind kind;
		// Adam / SGD / Novograd
		AdamHyper adam;
		float sgd_learning_rate = 1e-3f, sgd_l2_reg = 1e-8f;  // sgd.h:139-140
		NovogradHyper novograd;
		uint32_t current_step = 0;  // the bases' and Batched's own count
		float *m1 = nullptr, *m2 = nullptr;  // Adam: first / second moments; Novograd: m1 = first moments
		uint32_t* param_steps = nullptr;     // Adam
		float* layer_moments = nullptr;      // Novograd: two buffers of NOVOGRAD_MAX_LAYERS per-layer second moments; (current_step & 1) is current
		float* partials = nullptr;           // Novograd: NOVOGRAD_MAX_LAYERS * NOVOGRAD_REDUCE_BLOCKS
		// Ema
		float ema_decay = 0.99f;
		bool ema_full_precision = false;
		void* weights_ema = nullptr;  // T
		float* ema_tmp = nullptr;
		// ExponentialDecay (exponential_decay.h:153-160)
		float decay_base = 0.1f, lr_factor = 1.0f, base_lr = 0.0f;
		uint32_t decay_interval = 10000, decay_start = 10000, decay_end = 10000000;
		// Lookahead (lookahead.h:163-164)
		float alpha = 0.5f;
		uint32_t n_steps = 16;
		void* weights_lookahead = nullptr;  // T
		// Average (average.h:166)
		uint32_t n_samples = 128;
		void *weights_samples = nullptr, *weights_average = nullptr;  // T
		// Batched (batched.h:155)
		uint32_t batch_size_multiplier = 16;
		float* averaged_gradients = nullptr;
		void* averaged_gradients_half = nullptr;  // T
	};
	std::vector<Node> m_nodes;  // outermost first; the last one is the base
	uint32_t m_n = 0;
	NovogradLayers m_layers;
	uint32_t m_n_matrix = 0;
	bool m_allocated = false;
	bool m_fp32 = false;
	size_t value_bytes() const { return m_fp32 ? sizeof(float) : sizeof(half_t); }

	void apply(Node& node, const Json& config, bool creating);
	void release(Node& node);
	void allocate_average(Node& node);
	void step_node(size_t d, hipStream_t stream, float loss_scale, float* master, void* weights, const void* gradients, uint32_t begin, uint32_t end, bool advance);
	void step_node_f32(size_t d, hipStream_t stream, float loss_scale, float* weights, const float* gradients, uint32_t begin, uint32_t end, bool advance);
	void advance_exponential_decay(size_t d);
	uint32_t step_count(size_t d) const;
	void* custom_weights(size_t d) const;
	Json hyperparams(size_t d) const;
	void write_state(msgpack_detail::Writer& w, size_t d) const;
	void read_state(msgpack_detail::Reader& r, size_t d);
	float* novograd_moments(const Node& node) const { return node.layer_moments + (node.current_step & 1u) * NOVOGRAD_MAX_LAYERS; }
};

Json adam_hyperparams_json(const AdamHyper& h);  // adam.h:283-302

}  // namespace tcnn_hip

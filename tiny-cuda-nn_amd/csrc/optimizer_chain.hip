// optimizer_chain.hip -- see optimizer_chain.h.
#include "optimizer_chain.h"

#include <algorithm>
#include <stdexcept>

#include "device_alloc.h"
#include "host_common.h"
#include "model_desc.h"

namespace tcnn_hip {

using Kind = OptimizerChain::Kind;

const char* OptimizerChain::kind_name(Kind k) {
	switch (k) {
		case Kind::Adam: return "Adam";
		case Kind::SGD: return "SGD";
		case Kind::Novograd: return "Novograd";
		case Kind::Ema: return "EMA";  // ema.h:183
		case Kind::ExponentialDecay: return "ExponentialDecay";
		case Kind::Lookahead: return "Lookahead";
		case Kind::Average: return "Average";
		case Kind::Batched: return "Batched";
	}
	return "";
}

static bool is_base(Kind k) { return k == Kind::Adam || k == Kind::SGD || k == Kind::Novograd; }

static Kind kind_of(const std::string& otype) {  // optimizer.cu:50-86
	for (Kind k : {Kind::Adam, Kind::SGD, Kind::Novograd, Kind::Ema, Kind::ExponentialDecay, Kind::Lookahead, Kind::Average, Kind::Batched}) {
		if (equals_case_insensitive(otype, OptimizerChain::kind_name(k))) return k;
	}
	if (equals_case_insensitive(otype, "Composite")) {
		throw std::runtime_error("Optimizer 'Composite' is not supported by this build: it steps slices of the parameter buffer with several optimizer chains, this build steps the whole buffer with one.");
	}
	throw std::runtime_error("Optimizer '" + otype + "' is not available in this build (supported: Adam, SGD, Novograd, Ema, ExponentialDecay, Lookahead, Average, Batched).");
}

Json adam_hyperparams_json(const AdamHyper& h) {
	Json o = Json::object();
	o["otype"] = "Adam";
	o["beta1"] = h.beta1;
	o["beta2"] = h.beta2;
	o["epsilon"] = h.epsilon;
	o["learning_rate"] = h.learning_rate;
	o["l2_reg"] = h.l2_reg;
	o["adabound"] = h.adabound;
	o["relative_decay"] = h.relative_weight_decay;
	o["absolute_decay"] = h.absolute_weight_decay;
	o["clipping_magnitude"] = h.weight_clipping_magnitude;
	o["gradient_clipping_magnitude"] = h.gradient_clipping_magnitude;
	o["non_matrix_learning_rate_factor"] = h.non_matrix_learning_rate_factor;
	o["non_matrix_l2_reg"] = h.non_matrix_l2_reg;
	o["optimize_matrix_params"] = h.optimize_matrix_params;
	o["optimize_non_matrix_params"] = h.optimize_non_matrix_params;
	o["skip_zero_grad_non_matrix_params"] = h.skip_zero_grad_non_matrix_params;
	return o;
}

OptimizerChain::OptimizerChain(const Json& config, bool fp32) : m_fp32(fp32) {
	Json cur = config;
	for (;;) {
		const Kind kind = kind_of(cur.value("otype", "Adam"));
		for (const Node& n : m_nodes) {
			if (n.kind == kind) throw std::runtime_error(std::string("Optimizer: nested ") + kind_name(kind) + " inside " + kind_name(kind) + " is not supported");
		}
		Node node;
		node.kind = kind;
		m_nodes.push_back(node);
		if (is_base(kind)) break;
		cur = cur.value("nested", Json::object());
	}
	// inside-out, as the reference's constructors run: a wrapper reads its nested optimizer's learning rate (exponential_decay.h:52-53)
	std::vector<Json> configs;
	cur = config;
	for (size_t d = 0; d < m_nodes.size(); ++d) {
		configs.push_back(cur);
		cur = cur.value("nested", Json::object());
	}
	for (size_t d = m_nodes.size(); d-- > 0;) {
		apply(m_nodes[d], configs[d], /*creating=*/true);
		if (m_nodes[d].kind == Kind::ExponentialDecay) {
			m_nodes[d].lr_factor = 1.0f;
			float lr = 0.0f;
			for (size_t k = d + 1; k < m_nodes.size(); ++k) {  // the nested optimizer's learning_rate(): an inner ExponentialDecay cannot occur
				const Node& b = m_nodes[k];
				if (is_base(b.kind)) lr = b.kind == Kind::Adam ? b.adam.learning_rate : b.kind == Kind::SGD ? b.sgd_learning_rate : b.novograd.learning_rate;
			}
			m_nodes[d].base_lr = lr;
		}
	}
}

OptimizerChain::~OptimizerChain() {
	(void)hipDeviceSynchronize();
	for (Node& n : m_nodes) release(n);
}

void OptimizerChain::release(Node& n) {
	for (void** p : {(void**)&n.m1, (void**)&n.m2, (void**)&n.param_steps, (void**)&n.layer_moments, (void**)&n.partials, (void**)&n.weights_ema, (void**)&n.ema_tmp,
	                 (void**)&n.weights_lookahead, (void**)&n.weights_samples, (void**)&n.weights_average, (void**)&n.averaged_gradients, (void**)&n.averaged_gradients_half}) {
		if (*p) device_free(*p);
		*p = nullptr;
	}
}

// one node's own hyperparameters (update_hyperparams of its class in the reference); "nested" is walked by the caller
void OptimizerChain::apply(Node& n, const Json& c, bool creating) {
	switch (n.kind) {
		case Kind::Adam: parse_adam(n.adam, c); break;
		case Kind::SGD:  // sgd.h:113-121
			n.sgd_learning_rate = c.value("learning_rate", n.sgd_learning_rate);
			n.sgd_l2_reg = c.value("l2_reg", n.sgd_l2_reg);
			break;
		case Kind::Novograd:  // novograd.h:185-209
			n.novograd.beta1 = c.value("beta1", n.novograd.beta1);
			n.novograd.beta2 = c.value("beta2", n.novograd.beta2);
			n.novograd.epsilon = c.value("epsilon", n.novograd.epsilon);
			n.novograd.learning_rate = c.value("learning_rate", n.novograd.learning_rate);
			n.novograd.relative_weight_decay = c.value("relative_decay", n.novograd.relative_weight_decay);
			n.novograd.absolute_weight_decay = c.value("absolute_decay", n.novograd.absolute_weight_decay);
			break;
		case Kind::Ema:
			n.ema_decay = c.value("decay", n.ema_decay);
			if (creating) n.ema_full_precision = c.value("full_precision", n.ema_full_precision);
			break;
		case Kind::ExponentialDecay:
			n.decay_base = c.value("decay_base", n.decay_base);
			n.decay_interval = c.value("decay_interval", n.decay_interval);
			n.decay_start = c.value("decay_start", n.decay_start);
			n.decay_end = c.value("decay_end", n.decay_end);
			if (n.decay_interval == 0) throw std::runtime_error("ExponentialDecay: decay_interval must be positive");
			break;
		case Kind::Lookahead: {
			n.alpha = c.value("alpha", n.alpha);
			const uint32_t n_steps = c.value("n_steps", n.n_steps);
			if (n_steps == 0) throw std::runtime_error("Lookahead: n_steps must be positive");
			n.n_steps = n_steps;
			break;
		}
		case Kind::Average: {
			const uint32_t n_samples = c.value("n_samples", n.n_samples);
			if (n_samples == 0) throw std::runtime_error("Average: n_samples must be positive");
			const bool changed = c.contains("n_samples");
			n.n_samples = n_samples;
			if (changed && m_allocated) allocate_average(n);  // average.h:131-136: a new ring, zeroed
			break;
		}
		case Kind::Batched: {
			const uint32_t m = c.value("batch_size_multiplier", n.batch_size_multiplier);
			if (m == 0) throw std::runtime_error("Batched: batch_size_multiplier must be positive");
			n.batch_size_multiplier = m;
			break;
		}
	}
}

void OptimizerChain::update_hyperparams(const Json& config) {
	Json cur = config;
	for (size_t d = 0; d < m_nodes.size(); ++d) {
		Node& n = m_nodes[d];
		if (cur.contains("otype") && kind_of(cur.value("otype", "")) != n.kind) {
			throw std::runtime_error("update_hyperparams: optimizer structure does not match the trainer's");
		}
		const float lr_before = learning_rate();
		apply(n, cur, /*creating=*/false);
		if (is_base(n.kind) && learning_rate() != lr_before) {
			// the nested optimizer's learning rate was set directly: an ExponentialDecay above it schedules from the new value
			for (Node& w : m_nodes) {
				if (w.kind != Kind::ExponentialDecay) continue;
				w.base_lr = learning_rate();
				(n.kind == Kind::Adam ? n.adam.learning_rate : n.kind == Kind::SGD ? n.sgd_learning_rate : n.novograd.learning_rate) = w.base_lr * w.lr_factor;
			}
		}
		if (is_base(n.kind)) {
			if (cur.contains("nested")) throw std::runtime_error("update_hyperparams: optimizer structure does not match the trainer's");
			return;
		}
		if (!cur.contains("nested")) return;
		cur = cur.value("nested", Json::object());
	}
}

Json OptimizerChain::hyperparams(size_t d) const {
	const Node& n = m_nodes[d];
	Json o = Json::object();
	if (n.kind == Kind::Adam) {
		o = adam_hyperparams_json(n.adam);
		return o;
	}
	o["otype"] = kind_name(n.kind);
	if (!is_base(n.kind)) o["nested"] = hyperparams(d + 1);
	switch (n.kind) {
		case Kind::SGD:
			o["learning_rate"] = n.sgd_learning_rate;
			o["l2_reg"] = n.sgd_l2_reg;
			break;
		case Kind::Novograd:
			o["beta1"] = n.novograd.beta1;
			o["beta2"] = n.novograd.beta2;
			o["epsilon"] = n.novograd.epsilon;
			o["learning_rate"] = n.novograd.learning_rate;
			o["relative_decay"] = n.novograd.relative_weight_decay;
			o["absolute_decay"] = n.novograd.absolute_weight_decay;
			break;
		case Kind::Ema:
			o["decay"] = n.ema_decay;
			o["full_precision"] = n.ema_full_precision;
			break;
		case Kind::ExponentialDecay:
			o["decay_base"] = n.decay_base;
			o["decay_interval"] = n.decay_interval;
			o["decay_start"] = n.decay_start;
			o["decay_end"] = n.decay_end;
			break;
		case Kind::Lookahead:
			o["alpha"] = n.alpha;
			o["n_steps"] = n.n_steps;
			break;
		case Kind::Average: o["n_samples"] = n.n_samples; break;
		case Kind::Batched: o["batch_size_multiplier"] = n.batch_size_multiplier; break;
		default: break;
	}
	return o;
}

float OptimizerChain::learning_rate() const {
	const Node& b = m_nodes.back();
	return b.kind == Kind::Adam ? b.adam.learning_rate : b.kind == Kind::SGD ? b.sgd_learning_rate : b.novograd.learning_rate;
}
// reaches the base; an ExponentialDecay on the way rebases its schedule (exponential_decay.h:77-80)
void OptimizerChain::set_learning_rate(float v) {
	for (Node& n : m_nodes) {
		if (n.kind == Kind::ExponentialDecay) n.base_lr = v / n.lr_factor;
	}
	Node& b = m_nodes.back();
	(b.kind == Kind::Adam ? b.adam.learning_rate : b.kind == Kind::SGD ? b.sgd_learning_rate : b.novograd.learning_rate) = v;
}

bool OptimizerChain::contains(Kind k) const {
	return std::any_of(m_nodes.begin(), m_nodes.end(), [k](const Node& n) { return n.kind == k; });
}

uint32_t OptimizerChain::next_step_signature() const {
	uint32_t signature = 1u;
	for (size_t d = 0; d < m_nodes.size(); ++d) {
		const Node& n = m_nodes[d];
		if (n.kind == Kind::Lookahead) {
			const uint32_t current = step_count(d + 1);
			signature = signature * 4u + (current == 0 ? 2u : 0u) + (current % n.n_steps == 0 ? 1u : 0u);
		} else if (n.kind == Kind::Batched) {
			const bool nested_runs = (n.current_step + 1u) % n.batch_size_multiplier == 0;
			signature = signature * 2u + (nested_runs ? 1u : 0u);
			if (!nested_runs) break;  // nothing below it is launched
		}
	}
	return signature;
}

const char* OptimizerChain::ranged_refusal() const {
	for (const Node& n : m_nodes) {
		if (n.kind == Kind::Novograd || n.kind == Kind::Lookahead || n.kind == Kind::Average || n.kind == Kind::Batched) return kind_name(n.kind);
	}
	return nullptr;
}

uint32_t OptimizerChain::step_count(size_t d) const {
	for (; d < m_nodes.size(); ++d) {
		if (is_base(m_nodes[d].kind) || m_nodes[d].kind == Kind::Batched) return m_nodes[d].current_step;
	}
	return 0;
}

void* OptimizerChain::custom_weights(size_t d) const {
	for (; d < m_nodes.size(); ++d) {
		const Node& n = m_nodes[d];
		if (n.kind == Kind::Ema) return n.weights_ema;
		if (n.kind == Kind::Lookahead) return n.weights_lookahead;
		if (n.kind == Kind::Average) return n.weights_average;
	}
	return nullptr;
}

template <typename T>
static T* zeroed(size_t count) {
	T* p = device_malloc_n<T>(std::max<size_t>(count, 1));
	HIP_CHECK(hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T)));
	return p;
}
// a buffer of the chain's value type
static void* zeroed_values(size_t count, bool fp32) { return fp32 ? (void*)zeroed<float>(count) : (void*)zeroed<half_t>(count); }

void OptimizerChain::allocate_average(Node& n) {
	(void)hipDeviceSynchronize();
	device_free(n.weights_samples);
	device_free(n.weights_average);
	n.weights_samples = n.weights_average = nullptr;
	if ((uint64_t)m_n * n.n_samples > 0xFFFFFFFFull) throw std::runtime_error("Average: n_weights * n_samples exceeds 2^32 elements");
	n.weights_samples = zeroed_values((size_t)m_n * n.n_samples, m_fp32);
	n.weights_average = zeroed_values(m_n, m_fp32);
}

void OptimizerChain::allocate(uint32_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) {
	uint64_t n_matrix = 0;
	NovogradLayers layers;
	for (const auto& l : layer_sizes) {
		if (contains(Kind::Novograd)) {
			if (layers.n_layers >= NOVOGRAD_MAX_LAYERS) {
				throw std::runtime_error("Novograd: networks with more than " + std::to_string(NOVOGRAD_MAX_LAYERS) + " weight matrices are not supported by this build");
			}
			layers.begin[layers.n_layers++] = (uint32_t)n_matrix;
		}
		n_matrix += (uint64_t)l.first * l.second;
		if (n_matrix > n_weights) throw std::runtime_error("Optimizer::allocate: bad sizes");
		layers.begin[layers.n_layers] = (uint32_t)n_matrix;
	}
	(void)hipDeviceSynchronize();
	for (Node& n : m_nodes) release(n);
	m_n = n_weights;
	m_n_matrix = (uint32_t)n_matrix;
	m_layers = layers;
	m_allocated = true;
	for (Node& n : m_nodes) {
		n.current_step = 0;
		switch (n.kind) {
			case Kind::Adam:  // adam.h:136-156
				n.m1 = zeroed<float>(m_n);
				n.m2 = zeroed<float>(m_n);
				n.param_steps = zeroed<uint32_t>(m_n);
				break;
			case Kind::SGD: break;
			case Kind::Novograd:
				n.m1 = zeroed<float>(m_n);
				n.layer_moments = zeroed<float>(2 * NOVOGRAD_MAX_LAYERS);
				n.partials = zeroed<float>(NOVOGRAD_MAX_LAYERS * NOVOGRAD_REDUCE_BLOCKS);
				break;
			case Kind::Ema:  // ema.h:90-102
				n.weights_ema = zeroed_values(m_n, m_fp32);
				if (n.ema_full_precision && !m_fp32) n.ema_tmp = zeroed<float>(m_n);  // (an fp32 average is its own full-precision copy)
				break;
			case Kind::ExponentialDecay: break;
			case Kind::Lookahead: n.weights_lookahead = zeroed_values(m_n, m_fp32); break;
			case Kind::Average: allocate_average(n); break;
			case Kind::Batched:
				n.averaged_gradients = zeroed<float>(m_n);
				n.averaged_gradients_half = zeroed_values(m_n, m_fp32);
				break;
		}
	}
}

void OptimizerChain::step(hipStream_t stream, float loss_scale, float* master, void* weights, const void* gradients) {
	if (!m_n) return;
	step_node(0, stream, loss_scale, master, weights, gradients, 0, m_n, /*advance=*/true);
}

void OptimizerChain::step_range(hipStream_t stream, float loss_scale, float* master, void* weights, const void* gradients, uint32_t begin, uint32_t end, bool advance) {
	if (const char* who = ranged_refusal()) {
		throw std::runtime_error(std::string("optimizer_step_range: the ") + who + " optimizer cannot step a range of the parameters (it needs the whole gradient in one call)");
	}
	step_node(0, stream, loss_scale, master, weights, gradients, begin, std::min(end, m_n), advance);
}

// exponential_decay.h:59-70, step() == the nested count before this step
void OptimizerChain::advance_exponential_decay(size_t d) {
	Node& n = m_nodes[d];
	const uint32_t step = step_count(d + 1);
	if (step == 0) n.lr_factor = 1.0f;
	if (step >= n.decay_start && (step - n.decay_start) % n.decay_interval == 0 && step <= n.decay_end) n.lr_factor *= n.decay_base;
	Node& b = m_nodes.back();
	(b.kind == Kind::Adam ? b.adam.learning_rate : b.kind == Kind::SGD ? b.sgd_learning_rate : b.novograd.learning_rate) = n.base_lr * n.lr_factor;
}

void OptimizerChain::step_node(size_t d, hipStream_t stream, float loss_scale, float* master, void* weights_v, const void* gradients_v, uint32_t begin, uint32_t end,
                               bool advance) {
	Node& n = m_nodes[d];
	if (m_fp32) return step_node_f32(d, stream, loss_scale, master, (const float*)gradients_v, begin, end, advance);
	half_t* weights = (half_t*)weights_v;
	const half_t* gradients = (const half_t*)gradients_v;
	switch (n.kind) {
		case Kind::Adam:
			if (advance) ++n.current_step;  // adam.h:159
			adam_step(stream, n.adam, m_n, m_n_matrix, loss_scale, n.current_step, master, weights, const_cast<half_t*>(gradients) /* read only: no finalize rides along */,
			          n.m1, n.m2, n.param_steps, nullptr, nullptr, begin, end);
			break;
		case Kind::SGD:
			if (advance) ++n.current_step;  // sgd.h:82
			sgd_step(stream, m_n, loss_scale, n.sgd_learning_rate, n.sgd_l2_reg, master, weights, gradients, begin, end);
			break;
		case Kind::Novograd: {
			++n.current_step;  // novograd.h:122
			const float* in = n.layer_moments + ((n.current_step - 1u) & 1u) * NOVOGRAD_MAX_LAYERS;
			novograd_step(stream, m_layers, n.novograd, loss_scale, n.current_step == 1, master, weights, gradients, n.m1, in, novograd_moments(n), n.partials);
			break;
		}
		case Kind::Ema: {  // ema.h:102-136
			step_node(d + 1, stream, loss_scale, master, weights, gradients, begin, end, advance);
			const half_t* nested_custom = (const half_t*)custom_weights(d + 1);
			ema_step(stream, m_n, n.ema_decay, step_count(d + 1), nested_custom ? nested_custom : weights, (half_t*)n.weights_ema, n.ema_tmp, begin, end);
			break;
		}
		case Kind::ExponentialDecay:  // exponential_decay.h:59-70, step() == the nested count before this step
			if (advance) advance_exponential_decay(d);
			step_node(d + 1, stream, loss_scale, master, weights, gradients, begin, end, advance);
			break;
		case Kind::Lookahead: {  // lookahead.h:78-96; the copy is ordered on the stream (the step may be under graph capture)
			const uint32_t current = step_count(d + 1);
			if (current == 0) HIP_CHECK(hipMemcpyAsync(n.weights_lookahead, weights, (size_t)m_n * sizeof(half_t), hipMemcpyDeviceToDevice, stream));
			if (current % n.n_steps == 0) lookahead_step(stream, m_n, n.alpha, master, weights, (half_t*)n.weights_lookahead);
			step_node(d + 1, stream, loss_scale, master, weights, gradients, begin, end, advance);
			break;
		}
		case Kind::Average:  // average.h:81-91, slot = step() % n_samples AFTER the nested step
			step_node(d + 1, stream, loss_scale, master, weights, gradients, begin, end, advance);
			average_step(stream, m_n, n.n_samples, weights, (half_t*)n.weights_samples + (size_t)(step_count(d + 1) % n.n_samples) * m_n, (half_t*)n.weights_average);
			break;
		case Kind::Batched:  // batched.h:78-89
			batched_accumulate(stream, m_n, n.current_step % n.batch_size_multiplier == 0, n.batch_size_multiplier, gradients, n.averaged_gradients);
			++n.current_step;
			if (n.current_step % n.batch_size_multiplier == 0) {
				batched_cast(stream, m_n, n.averaged_gradients, (half_t*)n.averaged_gradients_half);
				step_node(d + 1, stream, loss_scale, master, weights, n.averaged_gradients_half, begin, end, advance);
			}
			break;
	}
}

// the same host logic for a chain over float: ONE weight vector (`weights`), float gradients, float wrapper state
void OptimizerChain::step_node_f32(size_t d, hipStream_t stream, float loss_scale, float* weights, const float* gradients, uint32_t begin, uint32_t end, bool advance) {
	Node& n = m_nodes[d];
	switch (n.kind) {
		case Kind::Adam:
			if (advance) ++n.current_step;  // adam.h:159
			adam_step_f32(stream, n.adam, m_n, m_n_matrix, loss_scale, n.current_step, weights, gradients, n.m1, n.m2, n.param_steps, begin, end);
			break;
		case Kind::SGD:
			if (advance) ++n.current_step;  // sgd.h:82
			sgd_step_f32(stream, m_n, loss_scale, n.sgd_learning_rate, n.sgd_l2_reg, weights, gradients, begin, end);
			break;
		case Kind::Novograd: {
			++n.current_step;  // novograd.h:122
			const float* in = n.layer_moments + ((n.current_step - 1u) & 1u) * NOVOGRAD_MAX_LAYERS;
			novograd_step_f32(stream, m_layers, n.novograd, loss_scale, n.current_step == 1, weights, gradients, n.m1, in, novograd_moments(n), n.partials);
			break;
		}
		case Kind::Ema: {  // ema.h:102-136
			step_node_f32(d + 1, stream, loss_scale, weights, gradients, begin, end, advance);
			const float* nested_custom = (const float*)custom_weights(d + 1);
			ema_step_f32(stream, m_n, n.ema_decay, step_count(d + 1), nested_custom ? nested_custom : weights, (float*)n.weights_ema, begin, end);
			break;
		}
		case Kind::ExponentialDecay:
			if (advance) advance_exponential_decay(d);
			step_node_f32(d + 1, stream, loss_scale, weights, gradients, begin, end, advance);
			break;
		case Kind::Lookahead: {  // lookahead.h:78-96
			const uint32_t current = step_count(d + 1);
			if (current == 0) HIP_CHECK(hipMemcpyAsync(n.weights_lookahead, weights, (size_t)m_n * sizeof(float), hipMemcpyDeviceToDevice, stream));
			if (current % n.n_steps == 0) lookahead_step_f32(stream, m_n, n.alpha, weights, (float*)n.weights_lookahead);
			step_node_f32(d + 1, stream, loss_scale, weights, gradients, begin, end, advance);
			break;
		}
		case Kind::Average:  // average.h:81-91, slot = step() % n_samples AFTER the nested step
			step_node_f32(d + 1, stream, loss_scale, weights, gradients, begin, end, advance);
			average_step_f32(stream, m_n, n.n_samples, weights, (float*)n.weights_samples + (size_t)(step_count(d + 1) % n.n_samples) * m_n, (float*)n.weights_average);
			break;
		case Kind::Batched:  // batched.h:78-89
			batched_accumulate_f32(stream, m_n, n.current_step % n.batch_size_multiplier == 0, n.batch_size_multiplier, gradients, n.averaged_gradients);
			++n.current_step;
			if (n.current_step % n.batch_size_multiplier == 0) {
				batched_cast_f32(stream, m_n, n.averaged_gradients, (float*)n.averaged_gradients_half);
				step_node_f32(d + 1, stream, loss_scale, weights, (const float*)n.averaged_gradients_half, begin, end, advance);
			}
			break;
	}
}

bool OptimizerChain::state_named(const std::string& name, void** ptr, size_t* count, size_t* elem_bytes) const {
	auto give = [&](void* p, size_t c, size_t e) {
		if (ptr) *ptr = p;
		if (count) *count = c;
		if (elem_bytes) *elem_bytes = e;
		return true;
	};
	for (const Node& n : m_nodes) {
		switch (n.kind) {
			case Kind::Adam:
				if (name == "first_moments") return give(n.m1, m_n, 4);
				if (name == "second_moments") return give(n.m2, m_n, 4);
				if (name == "param_steps") return give(n.param_steps, m_n, 4);
				break;
			case Kind::Novograd:
				if (name == "first_moments") return give(n.m1, m_n, 4);
				if (name == "per_layer_second_moments") return give(n.layer_moments ? novograd_moments(n) : nullptr, m_layers.n_layers, 4);
				break;
			case Kind::Ema:
				if (name == "weights_ema") return give(n.weights_ema, m_n, value_bytes());
				break;
			case Kind::Lookahead:
				if (name == "weights_lookahead") return give(n.weights_lookahead, m_n, value_bytes());
				break;
			case Kind::Average:
				if (name == "weights_samples") return give(n.weights_samples, (size_t)m_n * n.n_samples, value_bytes());
				if (name == "weights_average") return give(n.weights_average, m_n, value_bytes());
				break;
			case Kind::Batched:
				if (name == "averaged_gradients") return give(n.averaged_gradients, m_n, 4);
				if (name == "averaged_gradients_half") return give(n.averaged_gradients_half, m_n, value_bytes());
				break;
			default: break;
		}
	}
	return false;
}

// ---- snapshots: every optimizer's serialize() of the reference, keys in lexicographic order --------------------------------------------
static void write_device_blob(msgpack_detail::Writer& w, const void* device, size_t bytes) {
	if (w.count_only) {
		w.bin(nullptr, bytes);
		return;
	}
	std::vector<uint8_t> host(bytes);
	if (bytes) HIP_CHECK(hipMemcpy(host.data(), device, bytes, hipMemcpyDeviceToHost));
	w.bin(host.data(), bytes);
}
static void read_device_blob(msgpack_detail::Reader& r, void* device, size_t bytes, const char* what) {
	SnapshotBlob b;
	r.blob(b);
	if (b.size != bytes) throw std::runtime_error(std::string("Trainer: optimizer snapshot does not match the number of parameters (") + what + ")");
	if (bytes) HIP_CHECK(hipMemcpy(device, b.data, bytes, hipMemcpyHostToDevice));
}

void OptimizerChain::write_state(msgpack_detail::Writer& w, size_t d) const {
	const Node& n = m_nodes[d];
	const size_t nh = (size_t)m_n * value_bytes(), nf = (size_t)m_n * sizeof(float);  // nh: a buffer of the value type
	switch (n.kind) {
		case Kind::Adam:  // adam.h:304-312
			w.map(5);
			w.str("base_learning_rate"); w.real(double(n.adam.learning_rate));
			w.str("current_step"); w.uint(n.current_step);
			w.str("first_moments_binary"); write_device_blob(w, n.m1, nf);
			w.str("param_steps_binary"); write_device_blob(w, n.param_steps, nf);
			w.str("second_moments_binary"); write_device_blob(w, n.m2, nf);
			break;
		case Kind::SGD:  // sgd.h:131-136
			w.map(2);
			w.str("current_step"); w.uint(n.current_step);
			w.str("learning_rate"); w.real(double(n.sgd_learning_rate));
			break;
		case Kind::Novograd:  // novograd.h:223-230
			w.map(4);
			w.str("base_learning_rate"); w.real(double(n.novograd.learning_rate));
			w.str("current_step"); w.uint(n.current_step);
			w.str("first_moments_binary"); write_device_blob(w, n.m1, nf);
			w.str("per_layer_second_moments_binary"); write_device_blob(w, novograd_moments(n), (size_t)m_layers.n_layers * sizeof(float));
			break;
		case Kind::Ema:
			w.map(2);
			w.str("nested"); write_state(w, d + 1);
			w.str("weights_ema_binary"); write_device_blob(w, n.weights_ema, nh);
			break;
		case Kind::ExponentialDecay:
			w.map(3);
			w.str("learning_rate"); w.real(double(n.base_lr));
			w.str("learning_rate_factor"); w.real(double(n.lr_factor));
			w.str("nested"); write_state(w, d + 1);
			break;
		case Kind::Lookahead:  // lookahead.h:150-155
			w.map(2);
			w.str("nested"); write_state(w, d + 1);
			w.str("weights_lookahead_binary"); write_device_blob(w, n.weights_lookahead, nh);
			break;
		case Kind::Average:  // average.h:151-157
			w.map(3);
			w.str("nested"); write_state(w, d + 1);
			w.str("weights_average_binary"); write_device_blob(w, n.weights_average, nh);
			w.str("weights_samples_binary"); write_device_blob(w, n.weights_samples, nh * n.n_samples);
			break;
		case Kind::Batched:  // batched.h:138-145
			w.map(4);
			w.str("averaged_gradients_binary"); write_device_blob(w, n.averaged_gradients, nf);
			w.str("averaged_gradients_half_binary"); write_device_blob(w, n.averaged_gradients_half, nh);
			w.str("current_step"); w.uint(n.current_step);
			w.str("nested"); write_state(w, d + 1);
			break;
	}
}

void OptimizerChain::read_state(msgpack_detail::Reader& r, size_t d) {
	Node& n = m_nodes[d];
	const size_t nh = (size_t)m_n * value_bytes(), nf = (size_t)m_n * sizeof(float);  // nh: a buffer of the value type
	bool have_param_steps = false;
	for (uint32_t k = 0, m = r.map_header(); k < m; ++k) {
		const std::string key = r.str();
		if (key == "nested" && !is_base(n.kind) && r.is_map()) read_state(r, d + 1);
		else if (key == "current_step" && (is_base(n.kind) || n.kind == Kind::Batched)) n.current_step = uint32_t(r.unsigned_integer());
		else if (key == "base_learning_rate" && n.kind == Kind::Adam) n.adam.learning_rate = float(r.number());
		else if (key == "base_learning_rate" && n.kind == Kind::Novograd) n.novograd.learning_rate = float(r.number());
		else if (key == "learning_rate" && n.kind == Kind::SGD) n.sgd_learning_rate = float(r.number());
		else if (key == "learning_rate" && n.kind == Kind::ExponentialDecay) n.base_lr = float(r.number());
		else if (key == "learning_rate_factor" && n.kind == Kind::ExponentialDecay) n.lr_factor = float(r.number());
		else if (key == "first_moments_binary" && (n.kind == Kind::Adam || n.kind == Kind::Novograd)) read_device_blob(r, n.m1, nf, "first_moments");
		else if (key == "second_moments_binary" && n.kind == Kind::Adam) read_device_blob(r, n.m2, nf, "second_moments");
		else if (key == "param_steps_binary" && n.kind == Kind::Adam) { read_device_blob(r, n.param_steps, nf, "param_steps"); have_param_steps = true; }
		else if (key == "per_layer_second_moments_binary" && n.kind == Kind::Novograd) {
			// (current_step may follow in the document: both buffers take the moments, whichever is current)
			SnapshotBlob b;
			r.blob(b);
			if (b.size != (size_t)m_layers.n_layers * sizeof(float)) throw std::runtime_error("Trainer: optimizer snapshot does not match the network's layers (per_layer_second_moments)");
			for (uint32_t h = 0; h < 2 && b.size; ++h) HIP_CHECK(hipMemcpy(n.layer_moments + h * NOVOGRAD_MAX_LAYERS, b.data, b.size, hipMemcpyHostToDevice));
		}
		else if (key == "weights_ema_binary" && n.kind == Kind::Ema) {
			read_device_blob(r, n.weights_ema, nh, "weights_ema");
			if (n.ema_tmp) cast_f16_to_f32(nullptr, m_n, (const half_t*)n.weights_ema, n.ema_tmp);  // ema.h:200-203
		}
		else if (key == "weights_lookahead_binary" && n.kind == Kind::Lookahead) read_device_blob(r, n.weights_lookahead, nh, "weights_lookahead");
		else if (key == "weights_average_binary" && n.kind == Kind::Average) read_device_blob(r, n.weights_average, nh, "weights_average");
		else if (key == "weights_samples_binary" && n.kind == Kind::Average) read_device_blob(r, n.weights_samples, nh * n.n_samples, "weights_samples");
		else if (key == "averaged_gradients_binary" && n.kind == Kind::Batched) read_device_blob(r, n.averaged_gradients, nf, "averaged_gradients");
		else if (key == "averaged_gradients_half_binary" && n.kind == Kind::Batched) read_device_blob(r, n.averaged_gradients_half, nh, "averaged_gradients_half");
		else r.skip();
	}
	if (n.kind == Kind::Adam && !have_param_steps) HIP_CHECK(hipMemset(n.param_steps, 0, nf));  // adam.h:317-322: older snapshots carry none
}

}  // namespace tcnn_hip

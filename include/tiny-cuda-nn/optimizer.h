/*
 * tiny-cuda-nn/optimizer.h -- Optimizer<T> + create_optimizer<T>(json) (reference optimizer.h:40-99,
 * src/optimizer.cu:50-86).  The optimizers run inside the library: any order of the wrappers Ema, ExponentialDecay, Lookahead, Average,
 * Batched (each at most once) around one base out of Adam, SGD, Novograd.  This object carries the configuration to the Trainer built
 * from it and, once bound, reads the live state back.  Used on its own (allocate() + step(), optimizer.h:52-60) it owns the optimizer's
 * state over the caller's weight buffers (tcnn_create_optimizer).
 */
#pragma once
#include <tiny-cuda-nn/common.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace tcnn {

template <typename T>
class Optimizer {
public:
	explicit Optimizer(const json& params) : m_params(params) {}
	// optimizer.h:79: the live hyperparameters (the learning rate moves with an ExponentialDecay schedule) once the optimizer exists in the
	// library, the configuration before
	json hyperparams() const {
		if (m_tm) return json::parse(std::string(tcnn_trainer_hyperparams_json(m_tm))).value("optimizer", m_params);
		if (m_own) return json::parse(std::string(tcnn_optimizer_hyperparams_json(m_own)));
		return m_params;
	}
	void update_hyperparams(const json& params) {  // optimizer.h:77
		if (m_tm) {
			json wrapper = json::object();
			wrapper["optimizer"] = params;
			check(tcnn_trainer_update_hyperparams(m_tm, json_text(wrapper).c_str()));
		}
		if (m_own) check(tcnn_optimizer_update_hyperparams(m_own, json_text(params).c_str()));
		if (!m_tm && !m_own) m_params = params;
	}
	uint32_t step() const { return m_tm ? tcnn_trainer_optimizer_step_count(m_tm) : (m_own ? tcnn_optimizer_step_count(m_own) : 0u); }  // optimizer.h:66

	// optimizer.h:62-64: the base optimizer's learning rate, through every wrapper
	float learning_rate() const {
		json h = hyperparams();
		while (has(h, "nested")) h = h.value("nested", json::object());
		return h.value("learning_rate", 1e-3f);
	}
	void set_learning_rate(float val) {
		json leaf = json::object();
		leaf["learning_rate"] = val;
		update_hyperparams(with_leaf(hyperparams(), leaf));
	}

	// on its own (optimizer.h:52-60): layer_sizes = (rows, cols) of the weight matrices that lead the parameter buffer
	void allocate(uint32_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes = {}) {
		std::vector<uint32_t> rows, cols;
		for (const auto& l : layer_sizes) {
			rows.push_back(l.first);
			cols.push_back(l.second);
		}
		if (!m_own) check(tcnn_create_optimizer(json_text(m_params).c_str(), &m_own));
		check(tcnn_optimizer_allocate_layers(m_own, n_weights, rows.size(), rows.data(), cols.data()));
		m_n_weights = n_weights;
	}
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, T* weights, const T* gradients) {
		if (!m_own) throw std::runtime_error("Optimizer::step: allocate() first (an optimizer bound to a Trainer is stepped by the Trainer)");
		check(tcnn_optimizer_step(m_own, (tcnn_stream_t)stream, loss_scale, weights_full_precision, weights, gradients));
	}
	uint32_t n_weights() const { return m_tm ? (uint32_t)tcnn_trainer_n_params(m_tm) : m_n_weights; }
	// optimizer.h:70: the inference weights of the outermost wrapper that keeps any (Ema, Lookahead, Average), else nullptr
	T* custom_weights() const {
		if (m_own) return (T*)tcnn_optimizer_custom_weights(m_own);
		if (!m_tm) return nullptr;
		for (json h = hyperparams();; h = h.value("nested", json::object())) {
			const std::string otype = h.value("otype", "Adam");
			if (otype == "EMA" || otype == "Lookahead" || otype == "Average") return (T*)tcnn_trainer_params_inference(m_tm);
			if (!has(h, "nested")) return nullptr;
		}
	}
	// optimizer.h:72-75: a wrapper has one nested optimizer; `nested(0)` is a view of its configuration (the live chain is stepped,
	// updated and serialized through the outermost object)
	size_t n_nested() const { return has(m_params, "nested") ? 1 : 0; }
	std::shared_ptr<Optimizer<T>> nested(size_t idx = 0) const {
		if (idx != 0 || n_nested() == 0) throw std::runtime_error("Optimizer::nested: index out of range");
		return std::make_shared<Optimizer<T>>(hyperparams().value("nested", json::object()));
	}
	// optimizer.h:81-82 on its own: the state as the MessagePack bytes of the reference's JSON document (json::to_msgpack of serialize())
	std::vector<uint8_t> serialize() const {
		if (!m_own) throw std::runtime_error("Optimizer::serialize: allocate() first (a Trainer serializes the optimizer bound to it)");
		size_t n = 0;
		check(tcnn_optimizer_serialize(m_own, nullptr, 0, &n));
		std::vector<uint8_t> bytes(n);
		check(tcnn_optimizer_serialize(m_own, bytes.data(), bytes.size(), &n));
		return bytes;
	}
	void deserialize(const std::vector<uint8_t>& bytes) {
		if (!m_own) throw std::runtime_error("Optimizer::deserialize: allocate() first (a Trainer deserializes the optimizer bound to it)");
		check(tcnn_optimizer_deserialize(m_own, bytes.data(), bytes.size()));
	}
	~Optimizer() {
		if (m_own) tcnn_optimizer_destroy(m_own);
	}
	Optimizer(const Optimizer&) = delete;
	Optimizer& operator=(const Optimizer&) = delete;

	void bind(tcnn_trainable_model_t* tm) { m_tm = tm; }  // called by Trainer

private:
	// (spelled without json::contains, which older nlohmann::json releases lack)
	static bool has(const json& j, const char* key) { return j.is_object() && !j.value(key, json()).is_null(); }
	// `chain` with the innermost optimizer's hyperparameters replaced by `leaf`'s: only otypes and the leaf travel
	static json with_leaf(const json& chain, const json& leaf) {
		json out = json::object();
		if (has(chain, "otype")) out["otype"] = chain.value("otype", "Adam");
		if (has(chain, "nested")) {
			out["nested"] = with_leaf(chain.value("nested", json::object()), leaf);
		} else {
			out["learning_rate"] = leaf.value("learning_rate", 1e-3f);
		}
		return out;
	}

	json m_params;
	tcnn_trainable_model_t* m_tm = nullptr;
	tcnn_optimizer_t* m_own = nullptr;
	uint32_t m_n_weights = 0;
};

template <typename T>
Optimizer<T>* create_optimizer(const json& params) { return new Optimizer<T>(params); }

}  // namespace tcnn

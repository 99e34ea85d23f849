// trainer_snapshot.hip -- C ABI: Trainer::serialize / deserialize (document layout in snapshot_msgpack.h).
#include <cstring>
#include <string>
#include <vector>

#include "host_common.h"
#include "snapshot_msgpack.h"
#include "trainer_state.h"

using namespace tcnn_hip;

extern "C" {

// Trainer::serialize / deserialize, trainer.h:442-481 + adam.h:304-325; document layout in snapshot_msgpack.h.
static const char* const NATIVE_TYPE_NAME = HALF_IS_BF16 ? "__nv_bfloat16" : "__half";  // gpu_memory_json.h type strings

static Snapshot snapshot_shape(const tcnn_trainable_model* tm, bool with_optimizer) {
	const size_t n = tm->md.n_params();
	Snapshot s;
	s.n_params = n;
	s.params_type = NATIVE_TYPE_NAME;
	s.params.size = n * sizeof(half_t);
	s.has_optimizer = with_optimizer;
	if (tm->chain) {
		const OptimizerChain* chain = tm->chain.get();
		s.optimizer_writer = [chain](msgpack_detail::Writer& w) { chain->write_state(w); };
		return s;
	}
	s.current_step = tm->optimizer_step;
	s.base_learning_rate = tm->adam.learning_rate;
	s.first_moments.size = s.second_moments.size = n * sizeof(float);
	s.param_steps.size = n * sizeof(uint32_t);
	s.wrappers = tm->optimizer_order;
	if (tm->ema) s.weights_ema.size = n * sizeof(half_t);
	if (tm->lr_decay) {
		s.base_learning_rate = tm->adam.learning_rate;  // Adam's own (already scaled) rate, adam.h:307
		s.decay_learning_rate = tm->base_lr;
		s.decay_learning_rate_factor = tm->lr_factor;
	}
	return s;
}

int tcnn_trainer_serialize(tcnn_trainable_model_t* tm, int serialize_optimizer, void* buffer, size_t capacity, size_t* n_bytes) {
	TCNN_API_BEGIN
	Snapshot s = snapshot_shape(tm, serialize_optimizer != 0);
	const size_t needed = snapshot_encoded_size(s);
	if (n_bytes) *n_bytes = needed;
	if (buffer) {
		if (capacity < needed) throw std::runtime_error("tcnn_trainer_serialize: buffer too small (" + std::to_string(capacity) + " < " + std::to_string(needed) + " bytes)");
		HIP_CHECK(hipDeviceSynchronize());
		std::vector<uint8_t> host_params(s.params.size), host_m1, host_m2, host_steps, host_ema;
		HIP_CHECK(hipMemcpy(host_params.data(), tm->inference_params(), s.params.size, hipMemcpyDeviceToHost));  // trainer.h:448: params_inference
		s.params.data = host_params.data();
		if (s.has_optimizer && !tm->chain) {
			host_m1.resize(s.first_moments.size);
			host_m2.resize(s.second_moments.size);
			host_steps.resize(s.param_steps.size);
			HIP_CHECK(hipMemcpy(host_m1.data(), tm->m1, host_m1.size(), hipMemcpyDeviceToHost));
			HIP_CHECK(hipMemcpy(host_m2.data(), tm->m2, host_m2.size(), hipMemcpyDeviceToHost));
			if (tm->steps_form == ADAM_STEPS_DEFICITS8) {  // (the next optimizer step picks its representation again)
				step_counters_to_counter_form(tm, nullptr, tm->optimizer_step);
				HIP_CHECK(hipDeviceSynchronize());
			}
			HIP_CHECK(hipMemcpy(host_steps.data(), tm->steps, host_steps.size(), hipMemcpyDeviceToHost));
			if (tm->steps_form == ADAM_STEPS_DEFICITS32) {  // snapshots hold the counters themselves (adam.h:311)
				uint32_t* counters = (uint32_t*)host_steps.data();
				for (size_t i = 0; i < tm->md.n_params(); ++i) counters[i] = tm->optimizer_step - counters[i];
			}
			s.first_moments.data = host_m1.data();
			s.second_moments.data = host_m2.data();
			s.param_steps.data = host_steps.data();
			if (tm->ema) {
				host_ema.resize(s.weights_ema.size);
				HIP_CHECK(hipMemcpy(host_ema.data(), tm->params_ema, host_ema.size(), hipMemcpyDeviceToHost));
				s.weights_ema.data = host_ema.data();
			}
		}
		const std::vector<uint8_t> bytes = snapshot_encode(s);
		std::memcpy(buffer, bytes.data(), bytes.size());
	}
	TCNN_API_END
}

int tcnn_trainer_deserialize(tcnn_trainable_model_t* tm, const void* data, size_t n_bytes) {
	TCNN_API_BEGIN
	std::function<void(msgpack_detail::Reader&)> chain_reader;
	if (tm->chain) {
		HIP_CHECK(hipDeviceSynchronize());
		chain_reader = [tm](msgpack_detail::Reader& r) { tm->chain->read_state(r); };
	}
	const Snapshot s = snapshot_decode(static_cast<const uint8_t*>(data), n_bytes, chain_reader);
	const size_t n = tm->md.n_params();
	if (s.params_type == "float") {
		if (s.params.size != n * sizeof(float)) throw std::runtime_error("Can't set fp params because buffer has the wrong size.");  // trainer.h:410-412
		HIP_CHECK(hipMemcpy(tm->master, s.params.data, s.params.size, hipMemcpyHostToDevice));
		cast_master_to_params(tm, nullptr);
	} else if (s.params_type == NATIVE_TYPE_NAME) {
		if (s.params.size != n * sizeof(half_t)) throw std::runtime_error("Can't set params because buffer has the wrong size.");  // trainer.h:424-426
		HIP_CHECK(hipMemcpy(tm->params, s.params.data, s.params.size, hipMemcpyHostToDevice));
		tm->params_t_valid = false;
		cast_f16_to_f32(nullptr, n, tm->params, tm->master);
		HIP_CHECK(hipMemsetAsync(tm->grads, 0, n * sizeof(half_t), nullptr));
	} else {
		throw std::runtime_error(std::string("Trainer: snapshot parameters must be of type float of ") + NATIVE_TYPE_NAME);  // trainer.h:473
	}
	if (s.has_optimizer && tm->chain) {
		refresh_hyper_json(tm);
	} else if (s.has_optimizer) {
		if (!s.first_moments.present() || !s.second_moments.present() || s.first_moments.size != n * sizeof(float) || s.second_moments.size != n * sizeof(float))
			throw std::runtime_error("Trainer: optimizer snapshot does not match the number of parameters");
		HIP_CHECK(hipMemcpy(tm->m1, s.first_moments.data, s.first_moments.size, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(tm->m2, s.second_moments.data, s.second_moments.size, hipMemcpyHostToDevice));
		if (s.param_steps.present()) {  // adam.h:317-322: older snapshots carry no per-parameter steps
			if (s.param_steps.size != n * sizeof(uint32_t)) throw std::runtime_error("Trainer: optimizer snapshot does not match the number of parameters");
			HIP_CHECK(hipMemcpy(tm->steps, s.param_steps.data, s.param_steps.size, hipMemcpyHostToDevice));
		} else {
			HIP_CHECK(hipMemset(tm->steps, 0, n * sizeof(uint32_t)));
		}
		tm->steps_form = ADAM_STEPS_COUNTERS;  // the next optimizer step picks the representation again
		tm->optimizer_step = s.current_step;
		tm->adam.learning_rate = s.base_learning_rate;
		if (tm->ema) {  // ema.h:195-204
			if (!s.weights_ema.present() || s.weights_ema.size != n * sizeof(half_t)) throw std::runtime_error("Trainer: EMA snapshot does not match the number of parameters");
			HIP_CHECK(hipMemcpy(tm->params_ema, s.weights_ema.data, s.weights_ema.size, hipMemcpyHostToDevice));
			if (tm->ema_tmp) cast_f16_to_f32(nullptr, n, tm->params_ema, tm->ema_tmp);
		}
		if (tm->lr_decay && s.has_decay) {  // exponential_decay.h:144-148
			tm->base_lr = s.decay_learning_rate;
			tm->lr_factor = s.decay_learning_rate_factor;
		}
		refresh_hyper_json(tm);
	}
	HIP_CHECK(hipDeviceSynchronize());
	TCNN_API_END
}

}  // extern "C"

// trainer_optimizer.hip -- the trainer's optimizer: Adam inside optional Ema / ExponentialDecay wrappers on the trainer's own fields (with
// the fast paths that belong to Adam), any other chain through OptimizerChain -- its JSON, the (ranged) optimizer step, the representation
// of the per-parameter step counters.
#include <algorithm>
#include <string>

#include "host_common.h"
#include "trainer_state.h"

namespace tcnn_hip {

// optimizer.cu:50-86 for the optimizers of this build: Adam, optionally inside Ema / ExponentialDecay wrappers.
// `creating`: build the chain from the config; otherwise walk the existing chain (update_hyperparams, trainer.h:380-383).
// does the configuration name an optimizer that only OptimizerChain implements (or refuses by a name of its own)?
static bool names_chain_optimizer(const Json& opts) {
	Json cur = opts;
	for (size_t depth = 0; depth < 16 && cur.is_object(); ++depth) {
		const std::string otype = cur.value("otype", "Adam");
		for (const char* name : {"SGD", "Novograd", "Lookahead", "Average", "Batched", "Composite"}) {
			if (equals_case_insensitive(otype, name)) return true;
		}
		if (!cur.contains("nested")) break;
		cur = cur.value("nested", Json::object());
	}
	return false;
}

void apply_optimizer_json(tcnn_trainable_model* tm, const Json& opts, bool creating) {
	if (creating && names_chain_optimizer(opts)) {
		tm->chain = std::make_unique<OptimizerChain>(opts);
		return;
	}
	if (tm->chain) {
		tm->chain->update_hyperparams(opts);
		return;
	}
	if (!creating && names_chain_optimizer(opts)) throw std::runtime_error("update_hyperparams: optimizer structure does not match the trainer's");
	Json cur = opts;
	size_t depth = 0;
	for (;;) {
		std::string otype = cur.value("otype", creating ? "Adam" : (depth < tm->optimizer_order.size() ? tm->optimizer_order[depth] : "Adam"));
		if (equals_case_insensitive(otype, "Ema")) {
			if (creating) {
				if (tm->ema) throw std::runtime_error("Optimizer: nested Ema inside Ema is not supported");
				tm->ema = true;
				tm->optimizer_order.push_back("Ema");
			} else if (depth >= tm->optimizer_order.size() || tm->optimizer_order[depth] != "Ema") {
				throw std::runtime_error("update_hyperparams: optimizer structure does not match the trainer's");
			}
			tm->ema_decay = cur.value("decay", tm->ema_decay);
			if (creating) tm->ema_full_precision = cur.value("full_precision", tm->ema_full_precision);
		} else if (equals_case_insensitive(otype, "ExponentialDecay")) {
			if (creating) {
				if (tm->lr_decay) throw std::runtime_error("Optimizer: nested ExponentialDecay inside ExponentialDecay is not supported");
				tm->lr_decay = true;
				tm->optimizer_order.push_back("ExponentialDecay");
			} else if (depth >= tm->optimizer_order.size() || tm->optimizer_order[depth] != "ExponentialDecay") {
				throw std::runtime_error("update_hyperparams: optimizer structure does not match the trainer's");
			}
			tm->decay_base = cur.value("decay_base", tm->decay_base);
			tm->decay_interval = cur.value("decay_interval", tm->decay_interval);
			tm->decay_start = cur.value("decay_start", tm->decay_start);
			tm->decay_end = cur.value("decay_end", tm->decay_end);
			if (tm->decay_interval == 0) throw std::runtime_error("ExponentialDecay: decay_interval must be positive");
		} else if (equals_case_insensitive(otype, "Adam")) {
			const float lr_before = tm->adam.learning_rate;
			parse_adam(tm->adam, cur);
			if (tm->lr_decay) {
				if (creating) {
					tm->base_lr = tm->adam.learning_rate;  // exponential_decay.h:52
				} else if (tm->adam.learning_rate != lr_before) {
					tm->base_lr = tm->adam.learning_rate;  // the nested optimizer's learning rate was set directly
					tm->adam.learning_rate = tm->base_lr * tm->lr_factor;
				}
			}
			return;
		} else {
			throw std::runtime_error("Optimizer '" + otype + "' is not available in this build (supported: Adam, SGD, Novograd, Ema, ExponentialDecay, Lookahead, Average, Batched).");
		}
		if (!creating && !cur.contains("nested")) return;
		cur = cur.value("nested", Json::object());
		++depth;
	}
}

void refresh_hyper_json(tcnn_trainable_model* tm) {  // trainer.h:385-391, adam.h:283-302
	Json o = Json::object();
	o["otype"] = "Adam";
	o["beta1"] = tm->adam.beta1;
	o["beta2"] = tm->adam.beta2;
	o["epsilon"] = tm->adam.epsilon;
	o["learning_rate"] = tm->adam.learning_rate;
	o["l2_reg"] = tm->adam.l2_reg;
	o["adabound"] = tm->adam.adabound;
	o["relative_decay"] = tm->adam.relative_weight_decay;
	o["absolute_decay"] = tm->adam.absolute_weight_decay;
	o["clipping_magnitude"] = tm->adam.weight_clipping_magnitude;
	o["gradient_clipping_magnitude"] = tm->adam.gradient_clipping_magnitude;
	o["non_matrix_learning_rate_factor"] = tm->adam.non_matrix_learning_rate_factor;
	o["non_matrix_l2_reg"] = tm->adam.non_matrix_l2_reg;
	o["optimize_matrix_params"] = tm->adam.optimize_matrix_params;
	o["optimize_non_matrix_params"] = tm->adam.optimize_non_matrix_params;
	o["skip_zero_grad_non_matrix_params"] = tm->adam.skip_zero_grad_non_matrix_params;
	if (tm->lr_decay) o["learning_rate"] = tm->base_lr * tm->lr_factor;
	if (tm->chain) o = tm->chain->hyperparams();
	for (size_t k = tm->optimizer_order.size(); k-- > 0;) {  // wrap inside-out (ema.h:181-188, exponential_decay.h:116-125)
		Json wrapper = Json::object();
		if (tm->optimizer_order[k] == "Ema") {
			wrapper["otype"] = "EMA";
			wrapper["nested"] = o;
			wrapper["decay"] = tm->ema_decay;
			wrapper["full_precision"] = tm->ema_full_precision;
		} else {
			wrapper["otype"] = "ExponentialDecay";
			wrapper["nested"] = o;
			wrapper["decay_base"] = tm->decay_base;
			wrapper["decay_interval"] = tm->decay_interval;
			wrapper["decay_start"] = tm->decay_start;
			wrapper["decay_end"] = tm->decay_end;
		}
		o = wrapper;
	}
	Json l = Json::object();
	l["otype"] = loss_name(tm->loss);
	Json j = Json::object();
	j["otype"] = "Trainer";
	j["optimizer"] = o;
	j["loss"] = l;
	tm->hyper_json = j.dump();
}

}  // namespace tcnn_hip

using namespace tcnn_hip;

// Per-parameter step counters (adam.h:84) as counters or as deficits?  A stepped parameter costs 8 B of counter traffic in
// the first form and 4 B in the second, a skipped (zero-gradient) hash-table entry 0 B and 8 B.  With N samples touching
// 2^D corners per level, an entry of a level with T entries is skipped with probability exp(-N 2^D / T): deficits pay off
// below ~1/3, i.e. for N 2^D >= T at the largest level (the headline: 4 T).  TCNN_ADAM_STEP_DEFICITS=0/1 forces a form.
// The deficits are kept as BYTES (255 = the parameter's counter itself lives in the 32-bit array): one byte of bookkeeping per stepped
// parameter instead of four; the 32-bit deficit form remains for the optimizer step fused into the grid backward and for
// TCNN_ADAM_STEP_DEFICITS=1 (=0: counters, =2: bytes).
static int choose_step_representation(const tcnn_trainable_model* tm) {
	const int deficits = ADAM_STEPS_DEFICITS8;
	if (!tm->md.enc.is_grid()) return deficits;  // network weights are stepped every time
	const auto& g = tm->md.enc.grid;
	uint32_t largest = 0;
	for (uint32_t l = 0; l < g.n_levels; ++l) largest = std::max(largest, g.offset[l + 1] - g.offset[l]);
	const uint64_t batch = tm->global_batch ? tm->global_batch : tm->last_batch;  // the reduced gradient covers the global batch
	return (batch << g.n_dims) >= (uint64_t)largest ? deficits : ADAM_STEPS_COUNTERS;
}

namespace tcnn_hip {

void step_counters_to_counter_form(tcnn_trainable_model* tm, hipStream_t stream, uint32_t steps_done) {
	adam_convert_step_representation(stream, (uint32_t)tm->md.n_params(), steps_done, tm->steps, tm->step_deficits8, tm->steps_form, ADAM_STEPS_COUNTERS);
	tm->steps_form = ADAM_STEPS_COUNTERS;
}

}  // namespace tcnn_hip

// opens a new optimizer step: step counter, learning-rate schedule, representation of the per-parameter step counters
static void optimizer_advance(tcnn_trainable_model_t* tm, hipStream_t stream) {
	if (tm->lr_decay) {  // exponential_decay.h:59-70, with step() == the nested optimizer's step count before this step
		const uint32_t step = tm->optimizer_step;
		if (step == 0) tm->lr_factor = 1.0f;
		if (step >= tm->decay_start && (step - tm->decay_start) % tm->decay_interval == 0 && step <= tm->decay_end) tm->lr_factor *= tm->decay_base;
		tm->adam.learning_rate = tm->base_lr * tm->lr_factor;
	}
	++tm->optimizer_step;  // adam.h:159
	const int want = choose_step_representation(tm);
	if (want != tm->steps_form) {
		adam_convert_step_representation(stream, (uint32_t)tm->md.n_params(), tm->optimizer_step - 1u, tm->steps, tm->step_deficits8, tm->steps_form, want);
		tm->steps_form = want;
	}
}

// Adam over [begin, end) of the current optimizer step (optimizer_advance opened it), on `stream`
static void adam_range(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale, size_t begin, size_t end, bool counts, bool profile_any_stage) {
	// the trainer's 16-bit parameters are its rounded master weights unless a caller holds a pointer to them (params_exposed): Adam need
	// not read the skipped ones back (AdamCore::half_follows_master)
	const size_t n = tm->md.n_params();
	ProfScope prof(tm->profiler.get(), stream, STAGE_ADAM, counts, profile_any_stage);  // a ranged (bucketed) step is ONE optimizer step
	adam_step(stream, tm->adam, (uint32_t)n, (uint32_t)tm->md.n_mlp_params(), loss_scale, tm->optimizer_step, tm->master, tm->params, tm->grads,
	          tm->m1, tm->m2, tm->steps, tm->params_t_valid ? tm->params_t : nullptr, tm->md.has_network ? &tm->md.net.mlp : nullptr, (uint32_t)begin,
	          (uint32_t)end, tm->steps_form, tm->step_deficits8, /*half_follows_master=*/!tm->params_exposed,
	          begin == 0 && tm->pending_finalize.partials ? &tm->pending_finalize : nullptr);
	if (begin == 0) tm->pending_finalize = AdamFinalize();
	if (tm->ema) ema_step(stream, (uint32_t)n, tm->ema_decay, tm->optimizer_step, tm->params, tm->params_ema, tm->ema_tmp, (uint32_t)begin, (uint32_t)end);
}

namespace tcnn_hip {

void optimizer_step_ranges(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale, size_t n_ranges, const size_t* begins, const size_t* ends,
                           bool advance, bool opens_profiled_step, bool profile_any_stage) {
	const size_t n = tm->md.n_params();
	await_reduced_gradients(tm, stream);
	for (size_t r = 0; r < n_ranges; ++r) {
		if (begins[r] % 8 != 0 || begins[r] > std::min(ends[r], n)) throw std::runtime_error("optimizer_step_range: a range must start at a multiple of 8 and not end before it");
	}
	if (tm->chain) {  // finished 16-bit gradients in, `params` out: the transposed copy is stale afterwards
		const bool whole = n_ranges == 1 && begins[0] == 0 && ends[0] >= n && advance;
		ProfScope prof(tm->profiler.get(), stream, STAGE_ADAM, opens_profiled_step, profile_any_stage);
		if (whole) {
			tm->chain->step(stream, loss_scale, tm->master, tm->params, tm->grads);
		} else {
			for (size_t r = 0; r < n_ranges; ++r) {
				tm->chain->step_range(stream, loss_scale, tm->master, tm->params, tm->grads, (uint32_t)begins[r], (uint32_t)std::min(ends[r], n), advance && r == 0);
			}
		}
		tm->params_t_valid = false;
		return;
	}
	if (advance) optimizer_advance(tm, stream);
	for (size_t r = 0; r < n_ranges; ++r) {
		const size_t begin = begins[r], end = std::min(ends[r], n);
		if (begin == end) continue;
		adam_range(tm, stream, loss_scale, begin, end, /*counts=*/opens_profiled_step && r == 0, profile_any_stage);
	}
}

}  // namespace tcnn_hip

extern "C" {

// One optimizer step == calls whose ranges tile [0, n_params) exactly once, the range with begin == 0 first.
int tcnn_trainer_optimizer_step_range(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale, size_t begin, size_t end) {
	TCNN_API_BEGIN
	require_ranged_optimizer(tm, "optimizer_step_range");
	optimizer_step_ranges(tm, (hipStream_t)stream, loss_scale, 1, &begin, &end, /*advance=*/begin == 0, begin == 0);
	TCNN_API_END
}

// One optimizer step over the union of the given ranges only (a rank that owns a shard of the parameters, ZeRO-1 style:
// the other parameters' optimizer state is left untouched on this rank).
int tcnn_trainer_optimizer_step_ranges(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale, size_t n_ranges, const size_t* begins,
                                       const size_t* ends) {
	TCNN_API_BEGIN
	require_ranged_optimizer(tm, "optimizer_step_ranges");
	optimizer_step_ranges(tm, (hipStream_t)stream, loss_scale, n_ranges, begins, ends, /*advance=*/true, true);
	TCNN_API_END
}

}  // extern "C"

namespace tcnn_hip {

void require_ranged_optimizer(const tcnn_trainable_model* tm, const char* scheme) {
	const char* who = tm->chain ? tm->chain->ranged_refusal() : nullptr;
	if (who) throw std::runtime_error(std::string(scheme) + ": the " + who + " optimizer cannot step a range of the parameters (it needs the whole gradient in one call)");
}

void optimizer_step_all(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale) {
	const size_t begin = 0, end = tm->md.n_params();
	optimizer_step_ranges(tm, stream, loss_scale, 1, &begin, &end, /*advance=*/true, /*opens_profiled_step=*/true);
}

}  // namespace tcnn_hip

extern "C" {

int tcnn_trainer_optimizer_step(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale) {
	TCNN_API_BEGIN
	optimizer_step_all(tm, (hipStream_t)stream, loss_scale);  // (the whole vector in one call: every optimizer can)
	TCNN_API_END
}

// Adam's state for snapshots / sharded data parallelism: which = 0 first moments (fp32), 1 second moments (fp32),
// 2 per-parameter step counters (u32; *steps_are_deficits tells their representation, see tcnn_trainer_optimizer_step_range).
void* tcnn_trainer_optimizer_state(tcnn_trainable_model_t* tm, int which, int* steps_are_deficits) {
	if (tm->chain) {
		void* p = nullptr;
		if (steps_are_deficits) *steps_are_deficits = 0;
		if (tm->chain->base() != OptimizerChain::Kind::Adam) {
			set_last_error("tcnn_trainer_optimizer_state: the base optimizer is not Adam (use tcnn_trainer_optimizer_state_named)");
			return nullptr;
		}
		tm->chain->state_named(which == 0 ? "first_moments" : which == 1 ? "second_moments" : which == 2 ? "param_steps" : "", &p, nullptr, nullptr);
		return p;
	}
	if (which == 2 && tm->steps_form == ADAM_STEPS_DEFICITS8) {  // the byte form is the library's own business: hosts see counters
		(void)hipDeviceSynchronize();
		try {
			step_counters_to_counter_form(tm, nullptr, tm->optimizer_step);
		} catch (const std::exception& ex) {
			set_last_error(ex.what());
			return nullptr;
		}
		(void)hipDeviceSynchronize();
	}
	if (steps_are_deficits) *steps_are_deficits = tm->steps_form == ADAM_STEPS_DEFICITS32 ? 1 : 0;
	return which == 0 ? (void*)tm->m1 : which == 1 ? (void*)tm->m2 : which == 2 ? (void*)tm->steps : nullptr;
}

int tcnn_trainer_optimizer_state_named(tcnn_trainable_model_t* tm, const char* name, void** ptr, size_t* count, size_t* elem_bytes) {
	TCNN_API_BEGIN
	const std::string key = name ? name : "";
	const size_t n = tm->md.n_params();
	auto give = [&](void* p, size_t c, size_t e) {
		if (ptr) *ptr = p;
		if (count) *count = c;
		if (elem_bytes) *elem_bytes = e;
	};
	if (tm->chain) {
		if (!tm->chain->state_named(key, ptr, count, elem_bytes)) throw std::runtime_error("Optimizer: no state buffer named '" + key + "' in this optimizer");
	} else if (key == "first_moments") {
		give(tm->m1, n, 4);
	} else if (key == "second_moments") {
		give(tm->m2, n, 4);
	} else if (key == "param_steps") {
		int deficits = 0;
		void* steps = tcnn_trainer_optimizer_state(tm, 2, &deficits);
		if (!steps) return TCNN_ERROR;
		if (deficits) throw std::runtime_error("Optimizer: the step counters are held as deficits (tcnn_trainer_optimizer_state tells the form)");
		give(steps, n, 4);
	} else if (key == "weights_ema" && tm->ema) {
		give(tm->params_ema, n, 2);
	} else {
		throw std::runtime_error("Optimizer: no state buffer named '" + key + "' in this optimizer");
	}
	TCNN_API_END
}

int tcnn_trainer_update_hyperparams(tcnn_trainable_model_t* tm, const char* json) {
	TCNN_API_BEGIN
	const Json j = Json::parse(json);
	if (j.contains("optimizer")) apply_optimizer_json(tm, j.value("optimizer", Json::object()), /*creating=*/false);
	refresh_hyper_json(tm);
	TCNN_API_END
}
const char* tcnn_trainer_hyperparams_json(tcnn_trainable_model_t* tm) {
	refresh_hyper_json(tm);  // the learning rate moves with the ExponentialDecay schedule
	return tm->hyper_json.c_str();
}
uint32_t tcnn_trainer_optimizer_step_count(const tcnn_trainable_model_t* tm) { return tm->chain ? tm->chain->step_count() : tm->optimizer_step; }

}  // extern "C"

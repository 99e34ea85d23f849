// trainer_state.h -- the trainer object behind tcnn_trainable_model_t and its step context, and what the trainer's units
// (api_trainer, trainer_optimizer, trainer_exchange, trainer_snapshot) use of one another.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "direct_exchange.h"
#include "model_exec.h"
#include "optimizer_chain.h"

namespace tcnn_hip {

// what a forward pass of the trainer leaves for backward() and loss()
struct TrainContext {
	ForwardCtx model_ctx;
	Scratch output;       // half [n][padded]
	Scratch dL_doutput;   // half [n][padded]
	const half_t* dL_doutput_ptr = nullptr;  // == dL_doutput or the caller's external_dL_dy
	Scratch block_sums;   // fp32 partial loss sums
	uint32_t n_block_sums = 0;
	uint32_t n = 0;
	hipStream_t stream = nullptr;
};

struct Trainer {
	Model md;
	LossType loss = LossType::RelativeL2;
	AdamHyper adam;
	// wrapper optimizers around Adam (optimizers/ema.h, exponential_decay.h), outermost first
	std::vector<std::string> optimizer_order;  // e.g. {"Ema", "ExponentialDecay"}
	bool ema = false, ema_full_precision = false;
	float ema_decay = 0.99f;
	half_t* params_ema = nullptr;  // custom_weights(): the inference parameters while EMA is on (trainer.h:497-500)
	float* ema_tmp = nullptr;      // fp32 shadow of the average (full_precision)
	bool lr_decay = false;
	float decay_base = 0.1f, lr_factor = 1.0f, base_lr = 0.0f;
	uint32_t decay_interval = 10000, decay_start = 10000, decay_end = 10000000;
	// every other optimizer (SGD / Novograd bases, Lookahead / Average / Batched wrappers, in any chain): set instead of the fields above.
	// The Adam-only fast paths -- the weight-gradient slabs summed inside Adam's launch, the step counters' representations,
	// half_follows_master, the transposed copy kept current by the step -- belong to the fields above alone: a chain sees finished
	// 16-bit gradients and leaves `params_t` stale.  Ranged stepping: OptimizerChain::ranged_refusal.
	std::unique_ptr<OptimizerChain> chain;
	half_t* inference_params() const {  // trainer.h:497-500: the optimizer's custom_weights() if it has any
		if (chain) return chain->custom_weights() ? (half_t*)chain->custom_weights() : params;
		return ema ? params_ema : params;
	}
	bool has_custom_weights() const { return chain ? chain->custom_weights() != nullptr : ema; }
	// transposed copy of the network weights for the backward kernels; Adam keeps it current, anything else that writes
	// `params` invalidates it
	half_t* params_t = nullptr;
	bool params_t_valid = false;
	// a mutable pointer to `params` has left the library (tcnn_trainer_params / _params_inference): the caller may write
	// through it at any time, so from then on the transposed copy is rebuilt before every pass that needs it
	bool params_exposed = false;
	uint32_t optimizer_step = 0;
	Pcg32 rng;
	void* buffer = nullptr;  // [fp32 master | half params | half grads], trainer.h:76, 489-495
	float* master = nullptr;
	half_t* params = nullptr;
	half_t* grads = nullptr;
	float *m1 = nullptr, *m2 = nullptr;
	uint32_t* steps = nullptr;
	// `steps` holds the counters' deficits instead (elementwise_kernels.h: adam_flip_step_representation) while most
	// table entries are stepped every time; chosen per optimizer step from the last batch size, see choose_step_representation
	int steps_form = ADAM_STEPS_COUNTERS;  // AdamStepsForm of `steps` (+ `step_deficits8` for the byte form)
	uint8_t* step_deficits8 = nullptr;     // n_params bytes
	uint32_t last_batch = 0;
	uint64_t global_batch = 0;
	uint32_t lds_level_budget = 0;  // 0: default LDS slice size of the sliced grid backward
	std::string hyper_json;
	float* loss_scratch = nullptr;  // 1024 + 1 floats
	std::unique_ptr<Profiler> profiler;  // null unless tcnn_trainer_set_profiling enabled it
	// training_step on one GPU: the network kernel's fp32 weight-gradient slabs of THIS step, summed inside the optimizer's launch instead
	// of by a kernel of their own (AdamFinalize); set by training_step_fused for the optimizer step it runs itself, empty otherwise
	AdamFinalize pending_finalize;
	// training_step as ONE graph launch (tcnn_trainer_set_graph_capture; Trainer::training_step runs its passes under CudaGraph::capture_guard,
	// trainer.h:343-350, cuda_graph.h:65-155): every call re-records its launches into a graph, patches the instantiated graph with it and
	// launches that.  `graph_warm`: the shape (batch size and the flags that decide which scratch blocks a step takes) whose step has run
	// once outside a capture, so that the capture finds every block in the stream's cache and allocates nothing.
	bool graph_capture = false;
	hipGraphExec_t graph_exec = nullptr;
	uint64_t graph_warm = ~0ull;
	uint32_t max_level_generation = 0;  // counts the changes of the grid's max_level / max_level_gpu: part of a step's shape, so the step after one runs plainly
	uint32_t graph_signature = 0;  // OptimizerChain::next_step_signature() of the step `graph_exec` was instantiated from
	uint64_t graph_launches = 0, graph_instantiations = 0;
	// data-parallel hosts: called between backward and the optimizer (tcnn_trainer_set_gradient_exchange)
	void (*exchange)(void* user, void* gradients_fp16, size_t n_params, tcnn_stream_t stream) = nullptr;
	void* exchange_user = nullptr;
	// data-parallel hosts that overlap the exchange with the backward pass (tcnn_trainer_set_gradient_ready_callback,
	// tcnn_trainer_set_backward_level_groups, tcnn_trainer_enable_rccl)
	void (*gradients_ready)(void* user, size_t begin, size_t end, tcnn_stream_t stream) = nullptr;
	void* ready_user = nullptr;
	uint32_t backward_level_groups = 1u;
	void* rccl_comm = nullptr;  // ncclComm_t
	int rccl_ranks = 0;
	// gradient exchange over peer-mapped memory (direct_exchange.h; tcnn_trainer_direct_*)
	DirectExchange direct;
	// sharded exchange inside the library (tcnn_trainer_enable_rccl_sharded): reduce-scatter of every ready range -> Adam on this rank's
	// shards -> all-gather of the 16-bit parameters; -1: the all-reduce scheme
	int rccl_rank = -1;
	hipStream_t comm_stream = nullptr;
	std::vector<hipEvent_t> comm_events;
	size_t comm_events_used = 0;
	struct ReducedRange {
		size_t begin, end;
		hipEvent_t done;
		size_t shard = 0;  // sharded scheme: parameters per rank of this range's evenly divided part [begin, begin + shard * ranks); the rest is all-reduced
	};
	std::vector<ReducedRange> reduced;  // this step's ranges whose all-reduce is in flight on comm_stream, in issue order
	hipEvent_t comm_event() {
		if (comm_events_used == comm_events.size()) {
			hipEvent_t e;
			HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
			comm_events.push_back(e);
		}
		return comm_events[comm_events_used++];
	}
};

}  // namespace tcnn_hip

// the C ABI's opaque types
struct tcnn_train_context : tcnn_hip::TrainContext {};
struct tcnn_trainable_model : tcnn_hip::Trainer {};

namespace tcnn_hip {
// ---- what the trainer's units use of one another ----
// api_trainer.hip
void cast_master_to_params(tcnn_trainable_model* tm, hipStream_t stream);  // trainer.h:409-421
// trainer_optimizer.hip
void apply_optimizer_json(tcnn_trainable_model* tm, const Json& opts, bool creating);
void refresh_hyper_json(tcnn_trainable_model* tm);  // trainer.h:385-391, adam.h:283-302
// the per-parameter step counters as counters (what snapshots and hosts see); `steps_done` = optimizer steps completed
void step_counters_to_counter_form(tcnn_trainable_model* tm, hipStream_t stream, uint32_t steps_done);
// Optimizer::step over a set of parameter ranges [begin, end) (begins multiples of 8).  `advance`: this call opens a new
// optimizer step (step counter, learning-rate schedule, step-counter representation); the other calls of the same step
// (a data-parallel host steps each gradient bucket as soon as it is reduced) continue it.
// `profile_any_stage`: a profiler times the step whatever its stage filter says.
void optimizer_step_ranges(tcnn_trainable_model* tm, hipStream_t stream, float loss_scale, size_t n_ranges, const size_t* begins, const size_t* ends,
                           bool advance, bool opens_profiled_step, bool profile_any_stage = false);
void optimizer_step_all(tcnn_trainable_model* tm, hipStream_t stream, float loss_scale);  // one optimizer step over [0, n_params)
// data-parallel schemes that step by parameter range: throws, naming the optimizer, if the trainer's cannot (Novograd, Lookahead, Average, Batched)
void require_ranged_optimizer(const tcnn_trainable_model* tm, const char* scheme);
// trainer_exchange.hip
inline bool wants_ready_ranges(const tcnn_trainable_model* tm) { return tm->gradients_ready || tm->rccl_comm; }
void notify_gradients_ready(tcnn_trainable_model* tm, hipStream_t stream, size_t begin, size_t end);
// all-reduces this step started on the communication stream (tcnn_trainer_enable_rccl): `stream` continues behind them
void await_reduced_gradients(tcnn_trainable_model* tm, hipStream_t stream);
// The optimizer half of training_step.  With RCCL enabled every range whose all-reduce was started during the backward pass is
// stepped as soon as ITS collective has finished (the later ones are still on the wire); otherwise the host's exchange hook, then
// one optimizer step.
void finish_training_step(tcnn_trainable_model* tm, hipStream_t stream, float loss_scale);
}  // namespace tcnn_hip

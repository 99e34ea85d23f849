// api_trainer.hip -- C ABI: the Trainer (reference trainer.h:51-503): creation, forward / backward / training_step (fused, and captured
// into a graph), loss, inference, the *_matrices forms, parameter access, profiling.
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "device_alloc.h"
#include "host_common.h"
#include "switches.h"
#include "trainer_state.h"

namespace tcnn_hip {

void cast_master_to_params(tcnn_trainable_model* tm, hipStream_t stream) {  // trainer.h:409-421
	cast_f32_to_f16(stream, tm->md.n_params(), tm->master, tm->params);
	tm->params_t_valid = false;
	HIP_CHECK(hipMemsetAsync(tm->grads, 0, tm->md.n_params() * sizeof(half_t), stream));  // reset_param_gradients, trainer.h:419
}

}  // namespace tcnn_hip

using namespace tcnn_hip;

extern "C" {

// transposed network weights matching `params` (the pointer the pass is about to use)
static const half_t* trainer_params_t(tcnn_trainable_model* tm, hipStream_t stream, const half_t* params, Scratch& local) {
	if (!tm->md.has_network) return nullptr;
	if (params != tm->params || !tm->params_t) {  // EMA / foreign parameters: one-off transposition
		local = Scratch(stream, tm->md.n_mlp_params() * sizeof(half_t));
		mlp_transpose_weights(stream, tm->md.net.mlp, params, local.as<half_t>());
		return local.as<half_t>();
	}
	if (!tm->params_t_valid || tm->params_exposed) {
		mlp_transpose_weights(stream, tm->md.net.mlp, tm->params, tm->params_t);
		tm->params_t_valid = true;
	}
	return tm->params_t;
}

int tcnn_create_from_config(uint32_t n_input_dims, uint32_t n_output_dims, const char* config_json, uint32_t seed, tcnn_trainable_model_t** out) {
	TCNN_API_BEGIN
	const Json config = Json::parse(config_json);
	auto tm = std::make_unique<tcnn_trainable_model>();
	// config.h:53-63
	const Json loss_opts = config.value("loss", Json::object());
	const Json optimizer_opts = config.value("optimizer", Json::object());
	const Json network_opts = config.value("network", Json::object());
	const Json encoding_opts = config.value("encoding", Json::object());
	const std::string loss_type = loss_opts.value("otype", "RelativeL2");  // loss.cu:81-83
	tm->loss = string_to_loss(loss_type);
	apply_optimizer_json(tm.get(), optimizer_opts, /*creating=*/true);
	tm->md = make_nwie(n_input_dims, n_output_dims, encoding_opts, network_opts);
	refresh_hyper_json(tm.get());

	// Trainer ctor + initialize_params, trainer.h:51-87
	const size_t n = tm->md.n_params();
	tm->buffer = device_malloc(n * (sizeof(float) + 2 * sizeof(half_t)));
	HIP_CHECK(hipMemset(tm->buffer, 0, n * (sizeof(float) + 2 * sizeof(half_t))));
	tm->master = (float*)tm->buffer;
	tm->params = (half_t*)((char*)tm->buffer + sizeof(float) * n);
	tm->grads = tm->params + n;
	if (tm->chain) {  // Optimizer::allocate(n_params, layer_sizes), trainer.h:66: the network's weight matrices (object.h layer_sizes())
		std::vector<std::pair<uint32_t, uint32_t>> layers;
		if (tm->md.has_network) {
			const MlpMeta& m = tm->md.net.mlp;
			layers.emplace_back(m.width, m.in_width);
			for (uint32_t l = 0; l < m.n_hidden_matmuls; ++l) layers.emplace_back(m.width, m.width);
			layers.emplace_back(m.padded_out, m.width);
		}
		if (n > 0xFFFFFFFFull) throw std::runtime_error("Optimizer::allocate: bad sizes");
		tm->chain->allocate((uint32_t)n, layers);
	} else {
		tm->m1 = device_malloc_n<float>(n);  // adam.h:136-156
		tm->m2 = device_malloc_n<float>(n);
		tm->steps = device_malloc_n<uint32_t>(n);
		tm->step_deficits8 = device_malloc_n<uint8_t>(n);
		HIP_CHECK(hipMemset(tm->m1, 0, n * sizeof(float)));
		HIP_CHECK(hipMemset(tm->m2, 0, n * sizeof(float)));
		HIP_CHECK(hipMemset(tm->steps, 0, n * sizeof(uint32_t)));
	}
	if (tm->ema) {  // ema.h:90-102
		tm->params_ema = device_malloc_n<half_t>(n);
		HIP_CHECK(hipMemset(tm->params_ema, 0, n * sizeof(half_t)));
		if (tm->ema_full_precision) {
			tm->ema_tmp = device_malloc_n<float>(n);
			HIP_CHECK(hipMemset(tm->ema_tmp, 0, n * sizeof(float)));
		}
	}
	if (tm->md.has_network) tm->params_t = device_malloc_n<half_t>(tm->md.n_mlp_params());
	tm->loss_scratch = device_malloc_n<float>(1032);
	std::seed_seq seq{seed};
	std::vector<uint32_t> seeds(2);
	seq.generate(std::begin(seeds), std::end(seeds));
	tm->rng = Pcg32{seeds.front()};
	tm->md.initialize_params(nullptr, tm->rng, tm->master, 1.0f);
	cast_master_to_params(tm.get(), nullptr);
	HIP_CHECK(hipDeviceSynchronize());
	*out = tm.release();
	TCNN_API_END
}

void tcnn_trainable_model_destroy(tcnn_trainable_model_t* tm) {
	if (!tm) return;
	(void)hipDeviceSynchronize();
	direct_exchange_close(tm->direct);
	if (tm->direct.own_signals) (void)hipFree(tm->direct.own_signals);
	if (tm->direct.host_error) (void)hipHostFree((void*)tm->direct.host_error);
	device_free(tm->buffer);
	device_free(tm->m1);
	device_free(tm->m2);
	device_free(tm->steps);
	device_free(tm->step_deficits8);
	device_free(tm->params_t);
	device_free(tm->params_ema);
	device_free(tm->ema_tmp);
	device_free(tm->loss_scratch);
	for (hipEvent_t e : tm->comm_events) (void)hipEventDestroy(e);
	if (tm->comm_stream) (void)hipStreamDestroy(tm->comm_stream);
	if (tm->graph_exec) (void)hipGraphExecDestroy(tm->graph_exec);
	delete tm;
}

// Trainer::forward (trainer.h:97-131)
static void trainer_forward(tcnn_trainable_model_t* tm, hipStream_t stream, const IoLayout& layout, float loss_scale, uint32_t n, const float* input, const float* target,
                            const float* data_pdf, int use_inference_params, int prepare_input_gradients, const void* external_dL_dy,
                            tcnn_train_context_t** ctx_out) {
	Profiler* profiler = tm->profiler.get();
	const half_t* params = use_inference_params ? tm->inference_params() : tm->params;  // trainer.h:497-500 (EMA weights when Ema is on)
	auto c = std::make_unique<tcnn_train_context>();
	c->n = n;
	c->stream = stream;
	const uint32_t padded = tm->md.padded_output_width();
	c->output = Scratch(stream, (size_t)padded * n * sizeof(half_t));
	model_forward(stream, profiler, tm->md, layout, n, input, c->output.as<half_t>(), params, &c->model_ctx, prepare_input_gradients != 0);
	if (external_dL_dy) {  // trainer.h:124-128
		c->dL_doutput_ptr = (const half_t*)external_dL_dy;
	} else {
		if (!target) throw std::runtime_error("Trainer::forward: target must be given unless external_dL_dy is");
		c->dL_doutput = Scratch(stream, (size_t)padded * n * sizeof(half_t));
		c->dL_doutput_ptr = c->dL_doutput.as<half_t>();
		c->n_block_sums = loss_n_blocks(n, padded);
		c->block_sums = Scratch(stream, (size_t)c->n_block_sums * sizeof(float));
		const uint64_t n_total = (tm->global_batch ? tm->global_batch : (uint64_t)n) * tm->md.output_width();
		if (n_total > 0xFFFFFFFFull) throw std::runtime_error("Trainer::forward: batch too large");
		ProfScope prof(profiler, stream, STAGE_LOSS);
		loss_evaluate(stream, tm->loss, n, padded, tm->md.output_width(), loss_scale, c->output.as<half_t>(), target, data_pdf, nullptr,
		              c->dL_doutput.as<half_t>(), c->block_sums.as<float>(), (uint32_t)n_total);
	}
	*ctx_out = c.release();
}
int tcnn_trainer_forward(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale, uint32_t n, const float* input, const float* target,
                         const float* data_pdf, int use_inference_params, int prepare_input_gradients, const void* external_dL_dy,
                         tcnn_train_context_t** ctx_out) {
	TCNN_API_BEGIN
	trainer_forward(tm, (hipStream_t)stream, IoLayout::dense(tm->md), loss_scale, n, input, target, data_pdf, use_inference_params, prepare_input_gradients, external_dL_dy, ctx_out);
	TCNN_API_END
}

// Trainer::backward (trainer.h:133-148)
static void trainer_backward(tcnn_trainable_model_t* tm, hipStream_t stream, const IoLayout& layout, const tcnn_train_context_t* ctx, uint32_t n, const float* input,
                             float* dL_dinput, int use_inference_params, int gradient_mode) {
	tm->last_batch = n;
	if (!ctx) throw std::runtime_error("Trainer::backward: missing forward context");
	model_backward(stream, tm->profiler.get(), tm->md, layout, ctx->model_ctx, n, dL_dinput, ctx->dL_doutput_ptr, tm->grads, input, ctx->output.as<half_t>(),
	               use_inference_params ? tm->inference_params() : tm->params, gradient_mode,
	               tm->lds_level_budget);
}
int tcnn_trainer_backward(tcnn_trainable_model_t* tm, tcnn_stream_t stream, const tcnn_train_context_t* ctx, uint32_t n, const float* input,
                          float* dL_dinput, int use_inference_params, int gradient_mode) {
	TCNN_API_BEGIN
	trainer_backward(tm, (hipStream_t)stream, IoLayout::dense(tm->md), ctx, n, input, dL_dinput, use_inference_params, gradient_mode);
	TCNN_API_END
}

// A step that leaves the optimizer to a later call: the compute stream goes behind the all-reduces it started, so that whatever reads the
// gradient buffer next on that stream (the host's own optimizer_step, a copy of param_gradients) sees the reduced values.
static int settle_unstepped_reductions(tcnn_trainable_model_t* tm, hipStream_t stream, bool optimizer_ran) {
	if (optimizer_ran || !tm->rccl_comm) return TCNN_OK;
	TCNN_API_BEGIN
	await_reduced_gradients(tm, stream);
	TCNN_API_END
}
// The end of every training_step: the context goes to the caller, if there is one to take it and the step succeeded
static int conclude_training_step(tcnn_trainable_model_t* tm, hipStream_t stream, bool optimizer_ran, int r, tcnn_train_context_t* ctx, tcnn_train_context_t** ctx_out) {
	if (r == TCNN_OK) r = settle_unstepped_reductions(tm, stream, optimizer_ran);
	if (ctx_out && r == TCNN_OK) {
		*ctx_out = ctx;
	} else {
		delete ctx;
	}
	return r;
}
struct ReadyTrampoline {
	tcnn_trainable_model_t* tm;
	hipStream_t stream;
	static void call(void* self, size_t begin, size_t end) {
		auto* t = (ReadyTrampoline*)self;
		notify_gradients_ready(t->tm, t->stream, begin, end);
	}
};

// training_step fast path (g_fused_network_passes): encoding forward, ONE kernel for the network's forward + loss + backward, encoding
// backward.  Same results as forward() + backward() (tests/test_emu_kernels.py); the returned context carries the
// prediction, dL_doutput, the loss and the encoded input, but no hidden activations.
static int training_step_fused(tcnn_trainable_model_t* tm, hipStream_t stream, const IoLayout& layout, float loss_scale, uint32_t n, const float* input, const float* target,
                               const float* data_pdf, float* dL_dinput, int use_inference_params, int gradient_mode, bool run_optimizer,
                               const half_t* external_dL_dy, tcnn_train_context_t** ctx_out, bool context_wanted) {
	TCNN_API_BEGIN
	const half_t* params = use_inference_params ? tm->inference_params() : tm->params;
	Profiler* profiler = tm->profiler.get();
	const Model& md = tm->md;
	auto c = std::make_unique<tcnn_train_context>();
	c->n = n;
	c->stream = stream;
	ForwardCtx& fc = c->model_ctx;
	begin_pass(stream, md, n, &fc);
	const uint32_t padded = md.padded_output_width();
	const bool want_grads = gradient_mode != TCNN_GRADIENT_IGNORE;
	const bool accumulate = gradient_mode == TCNN_GRADIENT_ACCUMULATE;
	const EncodingDesc& e = md.enc;
	c->output = Scratch(stream, (size_t)padded * n * sizeof(half_t));
	if (external_dL_dy) {  // trainer.h:124-128: no loss is evaluated, the backward half continues from the caller's gradient
		c->dL_doutput_ptr = external_dL_dy;
	} else {
		c->dL_doutput = Scratch(stream, (size_t)padded * n * sizeof(half_t));
		c->dL_doutput_ptr = c->dL_doutput.as<half_t>();
	}
	const uint64_t n_total = (tm->global_batch ? tm->global_batch : (uint64_t)n) * md.output_width();
	if (n_total > 0xFFFFFFFFull) throw std::runtime_error("Trainer::forward: batch too large");
	if (n == 0) {
		*ctx_out = c.release();
		if (run_optimizer) optimizer_step_all(tm, stream, loss_scale);
		return TCNN_OK;
	}

	fc.enc = Scratch(stream, (size_t)e.padded_output_width * n * sizeof(half_t));
	// An Identity encoding that pads nothing is `(T)(x * scale + offset)` per element: the register-resident network kernel reads the caller's
	// fp32 matrix itself (MlpF32Input) and leaves the encoded matrix behind for the context -- no transpose kernel, no second pass over the input
	const bool plain_identity = e.kind == EncodingKind::Identity && e.n_dims == e.padded_output_width && layout.in_stride_i == e.n_dims && layout.in_stride_d == 1u;
	const bool input_by_network = plain_identity && !external_dL_dy && g_fused_identity_input.load() != 0 && n <= (1u << 25) &&
	                              mlp_train_f32_input_supported(md.net.mlp, n, tm->loss);
	if (!input_by_network) encoding_forward(stream, profiler, md, layout, n, input, params + md.n_mlp_params(), fc.enc.as<half_t>(), n, 1u, &fc, dL_dinput != nullptr);

	const bool need_denc = (want_grads && e.n_params > 0) || dL_dinput;
	Scratch denc;
	Scratch partials;
	{
		ProfScope prof(profiler, stream, STAGE_MLP_TRAIN);
		Scratch params_t_local;
		const half_t* params_t = trainer_params_t(tm, stream, params, params_t_local);
		const uint32_t n_partials = mlp_train_n_partials(md.net.mlp, n, external_dL_dy ? LossType::L2 : tm->loss);
		if (want_grads) partials = Scratch(stream, (size_t)n_partials * md.n_mlp_params() * sizeof(float));
		if (need_denc) denc = Scratch(stream, (size_t)e.padded_output_width * n * sizeof(half_t));
		MlpLossArgs la = {tm->loss, target, data_pdf, md.output_width(), loss_scale, (uint32_t)n_total};
		la.external_dL_doutput = external_dL_dy;
		if (!external_dL_dy) {  // Trainer::loss(ctx) has something to reduce
			c->n_block_sums = n_partials;
			c->block_sums = Scratch(stream, (size_t)n_partials * sizeof(float));
		}
		MlpF32Input f32_input;
		f32_input.x = input;
		f32_input.scale = e.id_scale;
		f32_input.offset = e.id_offset;
		f32_input.enc_out = context_wanted ? fc.enc.as<half_t>() : nullptr;  // (a context that is handed out holds the encoded input, whoever computed it)
		const SlabOrder order = mlp_train(stream, md.net.mlp, n, params, params_t, fc.enc.as<half_t>(), la, c->output.as<half_t>(),
		                                  external_dL_dy ? nullptr : c->dL_doutput.as<half_t>(), need_denc ? denc.as<half_t>() : nullptr,
		                                  want_grads ? partials.as<float>() : nullptr, external_dL_dy ? nullptr : c->block_sums.as<float>(),
		                                  input_by_network ? &f32_input : nullptr);
		// The slabs' sums: by the first workgroups of the optimizer's launch when this call runs the whole step itself on one GPU (nobody reads
		// the network's gradients between here and there: no exchange, no ready callback, no accumulation) -- by their own kernel otherwise.
		const bool sum_in_optimizer = want_grads && run_optimizer && !accumulate && !tm->chain && !tm->exchange && !tm->direct.active() && !wants_ready_ranges(tm) &&
		                              md.n_mlp_params() % 4 == 0 && g_finalize_in_optimizer.load() != 0;
		if (sum_in_optimizer) {
			tm->pending_finalize.partials = partials.as<float>();
			tm->pending_finalize.n_partials = n_partials;
			tm->pending_finalize.order = (uint32_t)order;
		} else if (want_grads) {
			mlp_finalize_gradients(stream, md.net.mlp, n_partials, partials.as<float>(), tm->grads, accumulate, order);
		}
	}
	struct DropPendingFinalize {  // (an exception between here and the optimizer must not leave a dangling slab pointer behind)
		tcnn_trainable_model_t* tm;
		~DropPendingFinalize() { tm->pending_finalize = AdamFinalize(); }
	} drop_pending_finalize = {tm};
	ReadyTrampoline tramp = {tm, stream};
	LevelGroups level_groups = {tm->backward_level_groups, want_grads && wants_ready_ranges(tm) ? &ReadyTrampoline::call : nullptr, &tramp};
	if (level_groups.ready) level_groups.ready(&tramp, 0, md.n_mlp_params());  // the network's gradients: the first range of the step
	if (need_denc) {
		encoding_backward(stream, profiler, md, layout, fc, n, dL_dinput, denc.as<half_t>(), n, 1u, tm->grads, want_grads, accumulate, input, tm->lds_level_budget, &level_groups);
	}
	*ctx_out = c.release();
	if (run_optimizer) finish_training_step(tm, stream, loss_scale);
	TCNN_API_END
}

// The step as one graph launch (opt-in; the reference's capture_guard).  Not on the null stream (cuda_graph.h:67-69), not inside a
// capture of the caller's (:72-76), not with an exchange / ready callback (their collectives live on other streams) or a profiler
// (its events would be recorded into the graph), and not before a plain step of the same shape has filled the stream's scratch cache.
static int training_step_fused_captured(tcnn_trainable_model_t* tm, tcnn_stream_t stream, const IoLayout& layout, float loss_scale, uint32_t n, const float* input, const float* target,
                                        const float* data_pdf, int run_optimizer, float* dL_dinput, int use_inference_params, int gradient_mode,
                                        const void* external_dL_dy, tcnn_train_context_t** ctx, bool context_wanted) {
	const uint64_t shape = (uint64_t)n | ((uint64_t)(dL_dinput != nullptr) << 32) | ((uint64_t)(gradient_mode & 3) << 33) | ((uint64_t)(use_inference_params != 0) << 35) |
	                       ((uint64_t)(external_dL_dy != nullptr) << 36) | ((uint64_t)context_wanted << 37) | ((uint64_t)(run_optimizer != 0) << 38) |
	                       ((uint64_t)(data_pdf != nullptr) << 39) | ((uint64_t)(tm->max_level_generation & 0xFFFFFFu) << 40);
	bool capture = tm->graph_capture && stream != nullptr && !tm->profiler && !tm->exchange && !tm->direct.active() && !wants_ready_ranges(tm) && n > 0 &&
	               tm->graph_warm == shape && (debug_launch_flags() & 1) == 0;
	if (capture) {
		hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
		if (hipStreamIsCapturing((hipStream_t)stream, &status) != hipSuccess || status != hipStreamCaptureStatusNone) capture = false;
	}
	if (capture && hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
		(void)hipGetLastError();
		capture = false;
	}
	// an optimizer chain's launches change from step to step (Lookahead's pull, Batched's nested step): the instantiated graph is only
	// patched by a step of the same launches, any other one instantiates anew
	const uint32_t signature = tm->chain && run_optimizer ? tm->chain->next_step_signature() : 0u;
	int r = training_step_fused(tm, (hipStream_t)stream, layout, loss_scale, n, input, target, data_pdf, dL_dinput, use_inference_params, gradient_mode,
	                            run_optimizer != 0, (const half_t*)external_dL_dy, ctx, context_wanted);
	if (capture) {
		hipGraph_t graph = nullptr;
		const hipError_t ended = hipStreamEndCapture((hipStream_t)stream, &graph);  // (always: the stream must leave capture mode, whatever happened)
		if (r == TCNN_OK && (ended != hipSuccess || !graph)) {
			(void)hipGetLastError();
			tm->graph_capture = false;  // the step was recorded, not run, and its host-side effects (step count) have happened: say so loudly, once
			set_last_error(std::string("training_step: capturing the step into a graph failed (") + hipGetErrorString(ended) + "); graph capture is switched off, this step did not run");
			r = TCNN_ERROR;
		}
		if (r == TCNN_OK) {
			if (tm->graph_exec && signature != tm->graph_signature) {
				(void)hipGraphExecDestroy(tm->graph_exec);
				tm->graph_exec = nullptr;
			}
			tm->graph_signature = signature;
			if (tm->graph_exec) {  // patch the instantiated graph with this step's arguments (cuda_graph.h:118-138); a new topology re-instantiates
				hipGraphNode_t error_node = nullptr;
				hipGraphExecUpdateResult result = hipGraphExecUpdateSuccess;
				if (hipGraphExecUpdate(tm->graph_exec, graph, &error_node, &result) != hipSuccess || result != hipGraphExecUpdateSuccess) {
					(void)hipGetLastError();
					(void)hipGraphExecDestroy(tm->graph_exec);
					tm->graph_exec = nullptr;
				}
			}
			hipError_t e = hipSuccess;
			if (!tm->graph_exec) {
				e = hipGraphInstantiate(&tm->graph_exec, graph, nullptr, nullptr, 0);
				++tm->graph_instantiations;
			}
			if (e == hipSuccess) e = hipGraphLaunch(tm->graph_exec, (hipStream_t)stream);
			if (e != hipSuccess) {
				(void)hipGetLastError();
				tm->graph_capture = false;
				set_last_error(std::string("training_step: launching the captured step failed (") + hipGetErrorString(e) + "); graph capture is switched off, this step did not run");
				r = TCNN_ERROR;
			} else {
				++tm->graph_launches;
			}
		}
		if (graph) (void)hipGraphDestroy(graph);
	} else if (r == TCNN_OK) {
		tm->graph_warm = shape;
	}
	return r;
}

static int try_finish_training_step(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale) {
	TCNN_API_BEGIN
	finish_training_step(tm, stream, loss_scale);
	TCNN_API_END
}

// Trainer::training_step (trainer.h:254-353)
static int training_step(tcnn_trainable_model_t* tm, tcnn_stream_t stream, const IoLayout& layout, uint32_t n, const float* input, const float* target,
                         const float* data_pdf, int run_optimizer, float* dL_dinput, int use_inference_params, int gradient_mode,
                         const void* external_dL_dy, tcnn_train_context_t** ctx_out) {
	const float loss_scale = LOSS_SCALE_FP16;  // trainer.h:265
	tm->last_batch = n;
	// all-reduces of an earlier step(run_optimizer = false) may still be on the communication stream: this step's backward pass writes
	// the same gradient buffer and re-records the same events, so the compute stream goes behind them first
	try {
		await_reduced_gradients(tm, (hipStream_t)stream);
	} catch (const std::exception& ex) {
		set_last_error(ex.what());
		return TCNN_ERROR;
	}
	tm->comm_events_used = 0;
	if (tm->rccl_comm && tm->rccl_rank >= 0 && !run_optimizer && gradient_mode != TCNN_GRADIENT_IGNORE) {
		// after the reduce-scatter only this rank's shard of the gradient buffer holds sums: a host-side optimizer_step() over everything would be wrong
		set_last_error("training_step: the sharded exchange of tcnn_trainer_enable_rccl_sharded steps the optimizer inside training_step (run_optimizer must be true)");
		return TCNN_ERROR;
	}
	if (tm->rccl_comm && gradient_mode == TCNN_GRADIENT_ACCUMULATE) {
		// every all-reduce would sum the ranks' ACCUMULATED buffers again: the earlier micro-batches would be counted once per rank and step
		set_last_error("training_step: GradientMode::Accumulate cannot be combined with tcnn_trainer_enable_rccl (accumulate locally with the communicator switched off and reduce the buffer once)");
		return TCNN_ERROR;
	}
	tcnn_train_context_t* ctx = nullptr;
	int r;
	if (g_fused_network_passes.load() && tm->md.has_network && mlp_train_supported(tm->md.net.mlp) && (external_dL_dy || (target && loss_is_elementwise(tm->loss)))) {
		r = training_step_fused_captured(tm, stream, layout, loss_scale, n, input, target, data_pdf, run_optimizer, dL_dinput, use_inference_params, gradient_mode, external_dL_dy,
		                                 &ctx, /*context_wanted=*/ctx_out != nullptr);
		return conclude_training_step(tm, (hipStream_t)stream, run_optimizer != 0, r, ctx, ctx_out);
	}
	try {
		trainer_forward(tm, (hipStream_t)stream, layout, loss_scale, n, input, target, data_pdf, use_inference_params, dL_dinput != nullptr, external_dL_dy, &ctx);
		trainer_backward(tm, (hipStream_t)stream, layout, ctx, n, input, dL_dinput, use_inference_params, gradient_mode);
		r = TCNN_OK;
	} catch (const std::exception& ex) {
		set_last_error(ex.what());
		log_message(TCNN_LOG_ERROR, ex.what());
		r = TCNN_ERROR;
	}
	if (r == TCNN_OK && gradient_mode != TCNN_GRADIENT_IGNORE && wants_ready_ranges(tm)) {  // this path reports the whole buffer at once
		try {
			notify_gradients_ready(tm, (hipStream_t)stream, 0, tm->md.n_params());
		} catch (const std::exception& ex) {
			set_last_error(ex.what());
			r = TCNN_ERROR;
		}
	}
	if (r == TCNN_OK && run_optimizer) r = try_finish_training_step(tm, (hipStream_t)stream, loss_scale);
	return conclude_training_step(tm, (hipStream_t)stream, run_optimizer != 0, r, ctx, ctx_out);
}
int tcnn_trainer_training_step(tcnn_trainable_model_t* tm, tcnn_stream_t stream, uint32_t n, const float* input, const float* target,
                               const float* data_pdf, int run_optimizer, float* dL_dinput, int use_inference_params, int gradient_mode,
                               const void* external_dL_dy, tcnn_train_context_t** ctx_out) {
	return training_step(tm, stream, IoLayout::dense(tm->md), n, input, target, data_pdf, run_optimizer, dL_dinput, use_inference_params, gradient_mode, external_dL_dy, ctx_out);
}

int tcnn_trainer_loss(tcnn_trainable_model_t* tm, tcnn_stream_t stream_, const tcnn_train_context_t* ctx, float* out_loss) {
	TCNN_API_BEGIN
	hipStream_t stream = (hipStream_t)stream_;
	if (!ctx || !ctx->block_sums.ptr) throw std::runtime_error("Trainer::loss: context holds no loss values (external_dL_dy was used)");
	reduce_sum(stream, ctx->block_sums.as<float>(), ctx->n_block_sums, tm->loss_scratch, tm->loss_scratch + 1024);
	HIP_CHECK(hipMemcpyAsync(out_loss, tm->loss_scratch + 1024, sizeof(float), hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipStreamSynchronize(stream));
	TCNN_API_END
}

void tcnn_train_context_destroy(tcnn_train_context_t* ctx) { delete ctx; }
const void* tcnn_train_context_output(const tcnn_train_context_t* ctx) { return ctx->output.ptr; }
const void* tcnn_train_context_dL_doutput(const tcnn_train_context_t* ctx) { return ctx->dL_doutput_ptr; }

int tcnn_network_inference(tcnn_trainable_model_t* tm, tcnn_stream_t stream_, uint32_t n, const float* input, float* output, int use_inference_params) {
	TCNN_API_BEGIN
	hipStream_t stream = (hipStream_t)stream_;
	inference_to_f32(stream, tm->md, IoLayout::dense(tm->md), n, input, use_inference_params ? tm->inference_params() : tm->params, output, tm->md.output_width(), 1u);
	TCNN_API_END
}

// ---- GPUMatrixDynamic-typed entry points (gpu_matrix.h:106-250): layout + stride of the caller's matrices honoured ----
static IoLayout layout_of(const tcnn_matrix_t* input, const tcnn_matrix_t* dL_dinput, uint32_t n_input_dims, uint32_t n) {
	auto check = [&](const tcnn_matrix_t* m, const char* what) {
		if (!m->data) throw std::runtime_error(std::string(what) + ": null matrix data");
		if (m->m != n_input_dims || m->n != n) throw std::runtime_error(std::string(what) + ": expected a " + std::to_string(n_input_dims) + " x " + std::to_string(n) + " matrix");
		const uint32_t min_stride = m->layout == TCNN_LAYOUT_COLUMN_MAJOR ? m->m : m->n;
		if (m->stride < min_stride) throw std::runtime_error(std::string(what) + ": stride smaller than the matrix' leading dimension");
	};
	IoLayout l;
	check(input, "input");
	const bool cm = input->layout == TCNN_LAYOUT_COLUMN_MAJOR;
	l.in_stride_i = cm ? input->stride : 1u;
	l.in_stride_d = cm ? 1u : input->stride;
	l.dx_stride_i = n_input_dims;
	l.dx_stride_d = 1u;
	if (dL_dinput) {
		check(dL_dinput, "dL_dinput");
		const bool dcm = dL_dinput->layout == TCNN_LAYOUT_COLUMN_MAJOR;
		l.dx_stride_i = dcm ? dL_dinput->stride : 1u;
		l.dx_stride_d = dcm ? 1u : dL_dinput->stride;
	}
	return l;
}
// target / data_pdf / external_dL_dy are GPUMatrix<T> (static column-major) in the reference's signatures (trainer.h:254-264)
static const void* dense_cm(const tcnn_matrix_t* m, uint32_t rows, uint32_t n, const char* what) {
	if (!m) return nullptr;
	if (m->layout != TCNN_LAYOUT_COLUMN_MAJOR || m->stride != m->m || m->m != rows || m->n != n) {
		throw std::runtime_error(std::string(what) + ": expected a dense column-major " + std::to_string(rows) + " x " + std::to_string(n) + " matrix");
	}
	return m->data;
}

// the loss's inputs of a *_matrices call as plain pointers
struct LossInputs {
	const void* external_dL_dy;
	const float *target, *data_pdf;
};
static LossInputs loss_inputs_of(const tcnn_trainable_model_t* tm, uint32_t n, const tcnn_matrix_t* target, const tcnn_matrix_t* data_pdf, const tcnn_matrix_t* external_dL_dy) {
	const void* ext = dense_cm(external_dL_dy, tm->md.padded_output_width(), n, "external_dL_dy");  // trainer.h:125-126
	// with an external gradient the loss is not evaluated: target and data_pdf are ignored, whatever they are (trainer.h:124-128)
	const void* tgt = ext ? (target && target->data ? target->data : nullptr) : dense_cm(target, tm->md.output_width(), n, "target");
	const void* pdf = ext ? nullptr : dense_cm(data_pdf, tm->md.output_width(), n, "data_pdf");
	return {ext, (const float*)tgt, (const float*)pdf};
}

int tcnn_trainer_training_step_matrices(tcnn_trainable_model_t* tm, tcnn_stream_t stream, const tcnn_matrix_t* input, const tcnn_matrix_t* target,
                                        const tcnn_matrix_t* data_pdf, int run_optimizer, const tcnn_matrix_t* dL_dinput, int use_inference_params,
                                        int gradient_mode, const tcnn_matrix_t* external_dL_dy, tcnn_train_context_t** ctx_out) {
	TCNN_API_BEGIN
	if (!input) throw std::runtime_error("training_step: input is required");
	const uint32_t n = input->n;
	const IoLayout layout = layout_of(input, dL_dinput, tm->md.n_input_dims, n);
	const LossInputs l = loss_inputs_of(tm, n, target, data_pdf, external_dL_dy);
	return training_step(tm, stream, layout, n, (const float*)input->data, l.target, l.data_pdf, run_optimizer, dL_dinput ? (float*)dL_dinput->data : nullptr,
	                     use_inference_params, gradient_mode, l.external_dL_dy, ctx_out);
	TCNN_API_END
}

// Trainer::forward / backward (trainer.h:97-148) with GPUMatrixDynamic inputs of either layout
int tcnn_trainer_forward_matrices(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale, const tcnn_matrix_t* input, const tcnn_matrix_t* target,
                                  const tcnn_matrix_t* data_pdf, int use_inference_params, int prepare_input_gradients, const tcnn_matrix_t* external_dL_dy,
                                  tcnn_train_context_t** ctx_out) {
	TCNN_API_BEGIN
	if (!input) throw std::runtime_error("forward: input is required");
	const uint32_t n = input->n;
	const IoLayout layout = layout_of(input, nullptr, tm->md.n_input_dims, n);
	const LossInputs l = loss_inputs_of(tm, n, target, data_pdf, external_dL_dy);
	trainer_forward(tm, (hipStream_t)stream, layout, loss_scale, n, (const float*)input->data, l.target, l.data_pdf, use_inference_params, prepare_input_gradients, l.external_dL_dy, ctx_out);
	TCNN_API_END
}
int tcnn_trainer_backward_matrices(tcnn_trainable_model_t* tm, tcnn_stream_t stream, const tcnn_train_context_t* ctx, const tcnn_matrix_t* input,
                                   const tcnn_matrix_t* dL_dinput, int use_inference_params, int gradient_mode) {
	TCNN_API_BEGIN
	if (!input) throw std::runtime_error("backward: input is required");
	const uint32_t n = input->n;
	const IoLayout layout = layout_of(input, dL_dinput, tm->md.n_input_dims, n);
	trainer_backward(tm, (hipStream_t)stream, layout, ctx, n, (const float*)input->data, dL_dinput ? (float*)dL_dinput->data : nullptr, use_inference_params, gradient_mode);
	TCNN_API_END
}

int tcnn_network_inference_matrices(tcnn_trainable_model_t* tm, tcnn_stream_t stream_, const tcnn_matrix_t* input, const tcnn_matrix_t* output,
                                    int use_inference_params) {
	TCNN_API_BEGIN
	if (!input || !output) throw std::runtime_error("inference: input and output are required");
	hipStream_t stream = (hipStream_t)stream_;
	const uint32_t n = input->n, width = tm->md.output_width();
	const IoLayout layout = layout_of(input, nullptr, tm->md.n_input_dims, n);
	if (output->m != width || output->n != n) throw std::runtime_error("inference: output must be n_output_dims x batch_size");  // object.h:221-222
	const bool cm = output->layout == TCNN_LAYOUT_COLUMN_MAJOR;
	if (output->stride < (cm ? output->m : output->n)) throw std::runtime_error("inference: output stride smaller than its leading dimension");
	inference_to_f32(stream, tm->md, layout, n, (const float*)input->data, use_inference_params ? tm->inference_params() : tm->params, (float*)output->data,
	                 cm ? output->stride : 1u, cm ? 1u : output->stride);
	TCNN_API_END
}

size_t tcnn_trainer_n_params(const tcnn_trainable_model_t* tm) { return tm->md.n_params(); }
// (mutable as well: a caller that writes the fp32 master weights through this pointer breaks "the 16-bit parameters are the rounded
// master weights" just like one that writes the 16-bit buffer, so it is treated the same way until tcnn_trainer_params_written)
float* tcnn_trainer_params_full_precision(tcnn_trainable_model_t* tm) {
	tm->params_exposed = true;
	return tm->master;
}
// read-only view of the same memory: the trainer's mode does not change (a logging / checkpointing host must not switch
// Adam's "16-bit weights follow the master weights" shortcut off for good)
const float* tcnn_trainer_params_full_precision_view(const tcnn_trainable_model_t* tm) { return tm->master; }
const void* tcnn_trainer_params_view(const tcnn_trainable_model_t* tm) { return tm->params; }
void* tcnn_trainer_params(tcnn_trainable_model_t* tm) {
	tm->params_exposed = true;  // a mutable pointer leaves the library: assume the caller writes through it, now or later
	return tm->params;
}
void* tcnn_trainer_params_inference(tcnn_trainable_model_t* tm) {
	if (!tm->has_custom_weights()) tm->params_exposed = true;  // the same buffer as `params` (trainer.h:497-500)
	return tm->inference_params();
}
void* tcnn_trainer_param_gradients(tcnn_trainable_model_t* tm) { return tm->grads; }

int tcnn_trainer_set_params_full_precision(tcnn_trainable_model_t* tm, const float* params, size_t n_params, int device_ptr) {
	TCNN_API_BEGIN
	if (n_params != tm->md.n_params()) throw std::runtime_error("Can't set fp params because buffer has the wrong size.");  // trainer.h:410-412
	HIP_CHECK(hipMemcpy(tm->master, params, sizeof(float) * n_params, device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
	cast_master_to_params(tm, nullptr);
	HIP_CHECK(hipDeviceSynchronize());
	TCNN_API_END
}

int tcnn_trainer_set_params(tcnn_trainable_model_t* tm, const void* params_fp16, size_t n_params, int device_ptr) {
	TCNN_API_BEGIN
	if (n_params != tm->md.n_params()) throw std::runtime_error("Can't set params because buffer has the wrong size.");  // trainer.h:424-426
	HIP_CHECK(hipMemcpy(tm->params, params_fp16, sizeof(half_t) * n_params, device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
	tm->params_t_valid = false;
	cast_f16_to_f32(nullptr, n_params, tm->params, tm->master);
	HIP_CHECK(hipMemsetAsync(tm->grads, 0, n_params * sizeof(half_t), nullptr));  // reset_param_gradients, trainer.h:437
	HIP_CHECK(hipDeviceSynchronize());
	TCNN_API_END
}

uint32_t tcnn_trainer_padded_output_width(const tcnn_trainable_model_t* tm) { return tm->md.padded_output_width(); }
uint32_t tcnn_trainer_n_mlp_params(const tcnn_trainable_model_t* tm) { return (uint32_t)tm->md.n_mlp_params(); }

// tcnn_trainer_params / _params_inference hand out a mutable pointer: from then on the transposed copy of the network weights is rebuilt
// before every pass.  A caller that has finished writing says so here; the copy is rebuilt once more and then trusted again.
// Which buffer is authoritative after direct writes: the 16-bit parameters (what the kernels compute with, what tcnn_trainer_params
// hands out).  The fp32 master weights are re-derived from them wherever the two disagree -- a parameter whose 16-bit value still IS
// its rounded master weight keeps the master's extra bits -- so a caller that wrote only the master buffer calls
// tcnn_trainer_set_params_full_precision instead.  After this call Adam's "16-bit weights follow the master weights" shortcut holds again.
int tcnn_trainer_params_written(tcnn_trainable_model_t* tm) {
	TCNN_API_BEGIN
	resync_master_from_half(nullptr, tm->md.n_params(), tm->params, tm->master);
	HIP_CHECK(hipDeviceSynchronize());
	tm->params_exposed = false;
	tm->params_t_valid = false;
	TCNN_API_END
}

int tcnn_trainer_set_global_batch_size(tcnn_trainable_model_t* tm, uint64_t global_batch_size) {
	tm->global_batch = global_batch_size;
	return TCNN_OK;
}

int tcnn_trainer_set_profiling(tcnn_trainable_model_t* tm, int enable, int only_stage) {
	TCNN_API_BEGIN
	if (!enable) {
		tm->profiler.reset();
	} else {
		tm->profiler = std::make_unique<Profiler>();
		tm->profiler->only_stage = only_stage;
		// events for the first steps exist before the caller's timed region begins (hipEventCreate costs host time: created on
		// first use they slowed a 20-step measurement by ~5 %)
		const size_t ahead = only_stage >= 0 ? 512 : 2048;
		for (size_t i = 0; i < ahead; ++i) (void)tm->profiler->get();
		tm->profiler->next = 0;
	}
	TCNN_API_END
}
int tcnn_trainer_n_stages(void) { return N_STAGES; }
const char* tcnn_trainer_stage_name(int stage) { return stage >= 0 && stage < N_STAGES ? STAGE_NAMES[stage] : ""; }
int tcnn_trainer_get_stage_times(tcnn_trainable_model_t* tm, double* total_ms, uint64_t* counts) {
	TCNN_API_BEGIN
	if (!tm->profiler) throw std::runtime_error("profiling is not enabled");
	tm->profiler->collect();
	for (int i = 0; i < N_STAGES; ++i) {
		total_ms[i] = tm->profiler->total_ms[i];
		counts[i] = tm->profiler->count[i];
	}
	TCNN_API_END
}
int tcnn_trainer_set_lds_level_budget(tcnn_trainable_model_t* tm, uint32_t bytes) {
	tm->lds_level_budget = bytes;
	return TCNN_OK;
}

// MultiLevelEncoding::set_max_level / max_level / set_max_level_gpu for the trainer's model.  A change takes effect at the next pass; with
// graph capture on, the first training_step after a change runs outside the graph (max_level_generation is part of the step's shape).
int tcnn_trainer_set_max_level(tcnn_trainable_model_t* tm, float value) {
	TCNN_API_BEGIN
	if (!tm) throw std::runtime_error("tcnn_trainer_set_max_level: null model");
	if (const int r = refuse_max_level(tm->md)) return r;
	if (tm->md.enc.grid.max_level != value) ++tm->max_level_generation;
	tm->md.enc.grid.max_level = value;
	TCNN_API_END
}
int tcnn_trainer_max_level(const tcnn_trainable_model_t* tm, float* out) {
	TCNN_API_BEGIN
	if (!tm || !out) throw std::runtime_error("tcnn_trainer_max_level: null argument");
	if (const int r = refuse_max_level(tm->md)) return r;
	*out = tm->md.enc.grid.max_level;
	TCNN_API_END
}
int tcnn_trainer_set_max_level_gpu(tcnn_trainable_model_t* tm, const float* device_ptr) {
	TCNN_API_BEGIN
	if (!tm) throw std::runtime_error("tcnn_trainer_set_max_level_gpu: null model");
	if (const int r = refuse_max_level(tm->md)) return r;
	if (tm->md.enc.max_level_gpu != device_ptr) ++tm->max_level_generation;
	tm->md.enc.max_level_gpu = device_ptr;
	TCNN_API_END
}

int tcnn_trainer_set_graph_capture(tcnn_trainable_model_t* tm, int enable) {
	TCNN_API_BEGIN
	if (!tm) throw std::runtime_error("tcnn_trainer_set_graph_capture: null model");
	tm->graph_capture = enable != 0;
	if (!enable && tm->graph_exec) {
		HIP_CHECK(hipDeviceSynchronize());
		(void)hipGraphExecDestroy(tm->graph_exec);
		tm->graph_exec = nullptr;
	}
	TCNN_API_END
}
int tcnn_trainer_graph_capture_stats(const tcnn_trainable_model_t* tm, uint64_t* launches, uint64_t* instantiations) {
	TCNN_API_BEGIN
	if (!tm) throw std::runtime_error("tcnn_trainer_graph_capture_stats: null model");
	if (launches) *launches = tm->graph_launches;
	if (instantiations) *instantiations = tm->graph_instantiations;
	TCNN_API_END
}

}  // extern "C"

// trainer_exchange.hip -- data-parallel gradient exchange of the trainer: host callbacks, RCCL (loaded at run time), the exchange over
// peer-mapped memory (direct_exchange.h), and the optimizer half of a training step that goes with each.
#include <dlfcn.h>

#include <string>
#include <vector>

#include "device_alloc.h"
#include "host_common.h"
#include "trainer_state.h"

using namespace tcnn_hip;
// RCCL, loaded at run time: the library links no collective library, a host that never asks for it never loads one
struct Rccl {
	void* handle = nullptr;
	int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
	int (*reduce_scatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;  // ncclReduceScatter(send, recv, recvcount, type, op, comm, stream)
	int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;           // ncclAllGather(send, recv, sendcount, type, comm, stream)
	int (*group_start)() = nullptr;
	int (*group_end)() = nullptr;
	int (*comm_get_async_error)(void*, int*) = nullptr;  // ncclCommGetAsyncError(comm, ncclResult_t*)
	const char* (*error_string)(int) = nullptr;
	static Rccl& get() {
		static Rccl r = [] {
			Rccl x;
			for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
				x.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
				if (x.handle) break;
			}
			if (x.handle) {
				x.all_reduce = (decltype(x.all_reduce))dlsym(x.handle, "ncclAllReduce");
				x.reduce_scatter = (decltype(x.reduce_scatter))dlsym(x.handle, "ncclReduceScatter");
				x.all_gather = (decltype(x.all_gather))dlsym(x.handle, "ncclAllGather");
				x.group_start = (decltype(x.group_start))dlsym(x.handle, "ncclGroupStart");
				x.group_end = (decltype(x.group_end))dlsym(x.handle, "ncclGroupEnd");
				x.comm_get_async_error = (decltype(x.comm_get_async_error))dlsym(x.handle, "ncclCommGetAsyncError");
				x.error_string = (decltype(x.error_string))dlsym(x.handle, "ncclGetErrorString");
			}
			return x;
		}();
		return r;
	}
};
constexpr int RCCL_SUM = 0, RCCL_HALF = 6, RCCL_BFLOAT16 = 9;  // rccl.h: ncclSum, ncclFloat16, ncclBfloat16
constexpr int RCCL_SUCCESS = 0, RCCL_IN_PROGRESS = 7;           // ncclSuccess, ncclInProgress
static void rccl_check(const Rccl& r, int rc, const char* what) {
	if (rc != RCCL_SUCCESS) throw std::runtime_error(std::string(what) + " failed: " + (r.error_string ? r.error_string(rc) : "?"));
}
// Collectives fail ASYNCHRONOUSLY (a peer that died, a link error): RCCL records the error on the communicator and the kernels already
// enqueued would wait forever.  Polled at every point where this library is about to put the compute stream behind a collective.
static void rccl_poll_async_error(tcnn_trainable_model* tm) {
	if (!tm->rccl_comm) return;
	const Rccl& r = Rccl::get();
	if (!r.comm_get_async_error) return;
	int state = RCCL_SUCCESS;
	const int rc = r.comm_get_async_error(tm->rccl_comm, &state);
	if (rc != RCCL_SUCCESS) throw std::runtime_error(std::string("ncclCommGetAsyncError failed: ") + (r.error_string ? r.error_string(rc) : "?"));
	if (state != RCCL_SUCCESS && state != RCCL_IN_PROGRESS) {
		throw std::runtime_error(std::string("RCCL reported an asynchronous error on the communicator: ") + (r.error_string ? r.error_string(state) : "?") +
		                         " (the gradient exchange of this step cannot complete; destroy the communicator and the trainer's rccl hook)");
	}
}

namespace tcnn_hip {

// Gradients [begin, end) of this step are final once the work enqueued on `stream` so far has run: tell the host (callback) and /
// or start their all-reduce on the communication stream, behind an event -- the rest of the backward pass keeps the compute
// stream busy meanwhile.
void notify_gradients_ready(tcnn_trainable_model* tm, hipStream_t stream, size_t begin, size_t end) {
	if (begin >= end) return;
	if (tm->gradients_ready) tm->gradients_ready(tm->ready_user, begin, end, stream);
	if (tm->rccl_comm) {
		Rccl& r = Rccl::get();
		rccl_poll_async_error(tm);
		hipEvent_t ready = tm->comm_event(), done = tm->comm_event();
		HIP_CHECK(hipEventRecord(ready, stream));
		HIP_CHECK(hipStreamWaitEvent(tm->comm_stream, ready, 0));
		const int type = HALF_IS_BF16 ? RCCL_BFLOAT16 : RCCL_HALF;
		size_t shard = 0;
		if (tm->rccl_rank >= 0) {
			// sharded: the part of the range that divides evenly over the ranks (shards of a multiple of 8 parameters, what the ranged optimizer
			// step needs) is reduce-scattered IN PLACE (recv = send + rank * shard: RCCL's in-place form), the remainder all-reduced
			const size_t P = (size_t)tm->rccl_ranks;
			shard = ((end - begin) / (8 * P)) * 8;
			if (shard) rccl_check(r, r.reduce_scatter(tm->grads + begin, tm->grads + begin + (size_t)tm->rccl_rank * shard, shard, type, RCCL_SUM, tm->rccl_comm, tm->comm_stream), "ncclReduceScatter");
			if (begin + shard * P < end) rccl_check(r, r.all_reduce(tm->grads + begin + shard * P, tm->grads + begin + shard * P, end - begin - shard * P, type, RCCL_SUM, tm->rccl_comm, tm->comm_stream), "ncclAllReduce");
		} else {
			rccl_check(r, r.all_reduce(tm->grads + begin, tm->grads + begin, end - begin, type, RCCL_SUM, tm->rccl_comm, tm->comm_stream), "ncclAllReduce");
		}
		HIP_CHECK(hipEventRecord(done, tm->comm_stream));
		tm->reduced.push_back({begin, end, done, shard});
	}
}

void await_reduced_gradients(tcnn_trainable_model_t* tm, hipStream_t stream) {
	for (const auto& r : tm->reduced) HIP_CHECK(hipStreamWaitEvent(stream, r.done, 0));
	tm->reduced.clear();
}

}  // namespace tcnn_hip

// reduce over the peers' mapped gradient buffers -> Adam on this rank's shard (the last rank's carries the remainder) -> push the stepped parameters
static void direct_exchange_and_step(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale) {
	DirectExchange& dx = tm->direct;
	Profiler* profiler = tm->profiler.get();
	direct_exchange_begin_step(dx);
	{
		{
			ProfScope prof(profiler, stream, STAGE_DX_WAIT_GRADS);
			direct_exchange_signal_wait(stream, dx, 0);
		}
		ProfScope prof(profiler, stream, STAGE_DX_REDUCE);
		direct_exchange_reduce_own(stream, dx);
	}
	std::vector<size_t> begins, ends;
	if (dx.own_count()) {
		begins.push_back(dx.own_begin);
		ends.push_back(dx.own_end);
	}
	// the exchange's Adam is one of its phases: timed whatever the profiler's stage filter says
	optimizer_step_ranges(tm, stream, loss_scale, begins.size(), begins.data(), ends.data(), /*advance=*/true, /*opens_profiled_step=*/true, /*profile_any_stage=*/true);
	{
		{
			ProfScope prof(profiler, stream, STAGE_DX_PUSH);
			direct_exchange_push_own(stream, dx);
		}
		ProfScope prof(profiler, stream, STAGE_DX_WAIT_PARAMS);
		direct_exchange_signal_wait(stream, dx, 1);
	}
	direct_exchange_finish_step(stream, dx);
	tm->params_t_valid = false;  // the transposed network weights were maintained for this rank's shard only
}

namespace tcnn_hip {

void finish_training_step(tcnn_trainable_model_t* tm, hipStream_t stream, float loss_scale) {
	if (tm->direct.active()) {
		direct_exchange_and_step(tm, stream, loss_scale);
		return;
	}
	if (tm->rccl_comm && !tm->reduced.empty()) {
		const std::vector<tcnn_trainable_model::ReducedRange> ranges = std::move(tm->reduced);
		tm->reduced.clear();
		if (ranges.front().begin != 0) throw std::runtime_error("training_step: the reduced gradient ranges do not start at parameter 0");
		rccl_poll_async_error(tm);
		if (tm->rccl_rank < 0) {  // the all-reduce scheme: every range is stepped as soon as its own collective has finished
			for (const auto& r : ranges) {
				HIP_CHECK(hipStreamWaitEvent(stream, r.done, 0));
				optimizer_step_ranges(tm, stream, loss_scale, 1, &r.begin, &r.end, /*advance=*/r.begin == 0, r.begin == 0);
			}
			return;
		}
		const Rccl& r = Rccl::get();
		const size_t P = (size_t)tm->rccl_ranks, me = (size_t)tm->rccl_rank;
		// ONE optimizer step over this rank's shards of all ranges (+ the remainders everyone steps), behind all reduce-scatters
		std::vector<size_t> begins, ends;
		for (const auto& rr : ranges) {
			HIP_CHECK(hipStreamWaitEvent(stream, rr.done, 0));
			if (rr.shard) {
				begins.push_back(rr.begin + me * rr.shard);
				ends.push_back(rr.begin + (me + 1) * rr.shard);
			}
			if (rr.begin + rr.shard * P < rr.end) {
				begins.push_back(rr.begin + rr.shard * P);
				ends.push_back(rr.end);
			}
		}
		optimizer_step_ranges(tm, stream, loss_scale, begins.size(), begins.data(), ends.data(), /*advance=*/true, /*opens_profiled_step=*/true);
		// all-gather of the stepped 16-bit parameters, in place (send = recv + rank * shard), on the communication stream behind the optimizer
		hipEvent_t stepped = tm->comm_event(), gathered = tm->comm_event();
		HIP_CHECK(hipEventRecord(stepped, stream));
		HIP_CHECK(hipStreamWaitEvent(tm->comm_stream, stepped, 0));
		const int type = HALF_IS_BF16 ? RCCL_BFLOAT16 : RCCL_HALF;
		if (r.group_start) rccl_check(r, r.group_start(), "ncclGroupStart");
		for (half_t* buf : {tm->params, tm->has_custom_weights() ? tm->inference_params() : (half_t*)nullptr}) {
			if (!buf) continue;
			for (const auto& rr : ranges) {
				if (rr.shard) rccl_check(r, r.all_gather(buf + rr.begin + me * rr.shard, buf + rr.begin, rr.shard, type, tm->rccl_comm, tm->comm_stream), "ncclAllGather");
			}
		}
		if (r.group_end) rccl_check(r, r.group_end(), "ncclGroupEnd");
		HIP_CHECK(hipEventRecord(gathered, tm->comm_stream));
		HIP_CHECK(hipStreamWaitEvent(stream, gathered, 0));  // whatever reads the parameters next on the compute stream sees everybody's shards
		tm->params_t_valid = false;  // the transposed network weights were maintained for this rank's shard only
		return;
	}
	if (tm->exchange) tm->exchange(tm->exchange_user, tm->grads, tm->md.n_params(), stream);
	optimizer_step_all(tm, stream, loss_scale);
}

}  // namespace tcnn_hip

extern "C" {

// Gradient exchange hook of a data-parallel C/C++ host: called by training_step(run_optimizer = true) between backward and
// the optimizer with the fp16 gradient buffer [network | encoding] and the stream the step runs on; the callback issues
// e.g. ncclAllReduce(grads, grads, n, ncclHalf, ncclSum, comm, stream).  The library itself links no collective library.
int tcnn_trainer_set_gradient_exchange(tcnn_trainable_model_t* tm, void (*exchange)(void* user, void* gradients_fp16, size_t n_params, tcnn_stream_t stream),
                                       void* user) {
	tm->exchange = exchange;
	tm->exchange_user = user;
	return TCNN_OK;
}

// Hosts that overlap the exchange with the backward pass.  `ready(user, begin, end, stream)` is called on the host, during
// training_step, as soon as the kernels that produce the gradients [begin, end) have been enqueued on `stream`: first the network's
// weights [0, n_network_params), then the encoding's levels in `n_groups` groups of consecutive levels (equal parameter counts;
// tcnn_trainer_set_backward_level_groups).  The ranges of one step tile [0, n_params) in ascending order, begins are multiples of 8.
int tcnn_trainer_set_gradient_ready_callback(tcnn_trainable_model_t* tm, void (*ready)(void* user, size_t begin, size_t end, tcnn_stream_t stream), void* user) {
	tm->gradients_ready = ready;
	tm->ready_user = user;
	return TCNN_OK;
}
int tcnn_trainer_set_backward_level_groups(tcnn_trainable_model_t* tm, uint32_t n_groups) {
	tm->backward_level_groups = n_groups ? n_groups : 1u;
	return TCNN_OK;
}
// Data parallelism without a callback: `nccl_comm` is the host's ncclComm_t for this rank (NULL switches it off again).  From then on
// training_step all-reduces (sum) every gradient range on an internal communication stream as soon as it is ready -- RCCL is loaded
// with dlopen at this point, the library does not link it -- and, with run_optimizer, steps each range when its own collective has
// finished.  The host sets the global batch size (tcnn_trainer_set_global_batch_size) so that the sum is the global gradient.
static void enable_rccl(tcnn_trainable_model_t* tm, void* nccl_comm, int n_ranks, int rank) {
	if (nccl_comm) {
		require_ranged_optimizer(tm, rank >= 0 ? "tcnn_trainer_enable_rccl_sharded" : "tcnn_trainer_enable_rccl");  // every reduced range is stepped on its own
		const Rccl& r = Rccl::get();
		if (!r.handle || !r.all_reduce) throw std::runtime_error("tcnn_trainer_enable_rccl: librccl.so could not be loaded");
		if (rank >= 0 && (!r.reduce_scatter || !r.all_gather)) throw std::runtime_error("tcnn_trainer_enable_rccl_sharded: librccl.so lacks ncclReduceScatter / ncclAllGather");
		if (n_ranks < 1 || rank >= n_ranks) throw std::runtime_error("tcnn_trainer_enable_rccl: rank / n_ranks out of range");
		if (!tm->comm_stream) HIP_CHECK(hipStreamCreateWithFlags(&tm->comm_stream, hipStreamNonBlocking));
	}
	tm->rccl_comm = nccl_comm;
	tm->rccl_ranks = n_ranks;
	tm->rccl_rank = nccl_comm ? rank : -1;
	tm->reduced.clear();
}
int tcnn_trainer_enable_rccl(tcnn_trainable_model_t* tm, void* nccl_comm, int n_ranks) {
	TCNN_API_BEGIN
	enable_rccl(tm, nccl_comm, n_ranks, -1);
	TCNN_API_END
}
// The sharded exchange inside the library (what tinycudann/parallel.py's "pipelined_sharded" does from Python): every ready gradient
// range is reduce-scattered; training_step(run_optimizer) then runs Adam on this rank's shard of every range only -- the optimizer, the
// largest HBM consumer of a step, shrinks by the number of ranks; fp32 master weights and Adam's moments of the other shards are never
// touched on this rank -- and all-gathers the 16-bit parameters (and the EMA weights of an Ema optimizer).  Same bytes on the wire as the
// all-reduce scheme; replicas cannot drift (everyone receives the same 16-bit parameters).  `rank`: this process's rank in `nccl_comm`.
int tcnn_trainer_enable_rccl_sharded(tcnn_trainable_model_t* tm, void* nccl_comm, int n_ranks, int rank) {
	TCNN_API_BEGIN
	if (nccl_comm && rank < 0) throw std::runtime_error("tcnn_trainer_enable_rccl_sharded: rank must be >= 0");
	enable_rccl(tm, nccl_comm, n_ranks, rank);
	TCNN_API_END
}

// ---- gradient exchange over peer-mapped memory (direct_exchange.h): every rank publishes IPC handles of its trainer buffer and of a small
// signal block, maps its peers', and from then on a step's exchange is: read the peers' shards of the own 1/P of the gradient buffer over all
// links at once, sum in fp32 in rank order, one rounding -> Adam on that shard -> write the stepped parameters into every peer's buffer.
int tcnn_trainer_direct_export(tcnn_trainable_model_t* tm, void* out, size_t capacity, size_t* n_bytes) {
	TCNN_API_BEGIN
	if (n_bytes) *n_bytes = sizeof(DirectExport);
	if (!out) return TCNN_OK;
	if (capacity < sizeof(DirectExport)) throw std::runtime_error("tcnn_trainer_direct_export: buffer too small");
	if (debug_alloc_mode() != DebugAlloc::Off) throw std::runtime_error("tcnn_trainer_direct_export: not available under TCNN_DEBUG_ALLOC (the trainer buffer must be a plain hipMalloc block)");
	require_ranged_optimizer(tm, "tcnn_trainer_direct_export");  // the direct exchange steps this rank's shard of the parameters
	if (tm->has_custom_weights()) throw std::runtime_error("tcnn_trainer_direct_export: Ema-wrapped optimizers are not supported by the direct exchange (use the sharded collective scheme)");
	HIP_CHECK(hipDeviceSynchronize());
	direct_exchange_export(tm->direct, tm->buffer, tm->params, tm->grads, tm->md.n_params(), *(DirectExport*)out);
	TCNN_API_END
}
int tcnn_trainer_direct_open(tcnn_trainable_model_t* tm, int rank, int n_ranks, const void* exports, size_t bytes_each) {
	TCNN_API_BEGIN
	if (bytes_each != sizeof(DirectExport) || !exports) throw std::runtime_error("tcnn_trainer_direct_open: exports must be n_ranks records of tcnn_trainer_direct_export's size");
	HIP_CHECK(hipDeviceSynchronize());
	direct_exchange_open(tm->direct, rank, n_ranks, (const DirectExport*)exports, tm->params, tm->grads);
	tm->params_exposed = true;  // peers write this rank's 16-bit parameters from now on: Adam must not re-derive skipped ones from its master weights
	TCNN_API_END
}
int tcnn_trainer_direct_close(tcnn_trainable_model_t* tm) {
	TCNN_API_BEGIN
	HIP_CHECK(hipDeviceSynchronize());
	direct_exchange_close(tm->direct);
	TCNN_API_END
}
// after training_step(run_optimizer = 0): the exchange + optimizer half of the step (training_step(run_optimizer = 1) does the same itself)
int tcnn_trainer_direct_exchange_and_step(tcnn_trainable_model_t* tm, tcnn_stream_t stream, float loss_scale) {
	TCNN_API_BEGIN
	if (!tm->direct.active()) throw std::runtime_error("tcnn_trainer_direct_exchange_and_step: tcnn_trainer_direct_open first");
	direct_exchange_and_step(tm, (hipStream_t)stream, loss_scale);
	TCNN_API_END
}
// 0: every wait of the exchange found its peers in time; 1 / 2: a wait for the peers' gradients / parameters timed out (synchronises)
int tcnn_trainer_direct_status(tcnn_trainable_model_t* tm, tcnn_stream_t stream, int* status) {
	TCNN_API_BEGIN
	*status = direct_exchange_status((hipStream_t)stream, tm->direct);
	TCNN_API_END
}

// Link check of an opened exchange (collective: same rounds and seed on every rank, between steps; overwrites the gradient buffer only).
// *mismatches: elements of this rank's buffer that did not hold the expected sum; *status as tcnn_trainer_direct_status.
int tcnn_trainer_direct_selftest(tcnn_trainable_model_t* tm, tcnn_stream_t stream, uint32_t rounds, uint32_t seed, uint64_t* mismatches, int* status) {
	TCNN_API_BEGIN
	if (!tm->direct.active()) throw std::runtime_error("tcnn_trainer_direct_selftest: tcnn_trainer_direct_open first");
	direct_exchange_selftest((hipStream_t)stream, tm->direct, rounds, seed, mismatches, status);
	TCNN_API_END
}

}  // extern "C"

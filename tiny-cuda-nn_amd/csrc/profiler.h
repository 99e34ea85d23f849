// profiler.h -- optional per-stage timing of a trainer's passes with HIP events (header-only; a null Profiler* means off).
#pragma once
#include <cstdint>
#include <vector>

#include "host_common.h"

namespace tcnn_hip {

// ------------------------------------------------------------------------------------------------
// optional per-stage timing with HIP events recorded on the stream the kernels are launched on
// (bench.py's roofline leg; off by default -- no events are recorded unless a trainer enables it)
// ------------------------------------------------------------------------------------------------
enum Stage : int {
	STAGE_GRID_FWD = 0,
	STAGE_MLP_FWD,
	STAGE_LOSS,
	STAGE_MLP_BWD,       // weight transpose + fused backward + finalize
	STAGE_MLP_TRAIN,     // training_step fast path: weight transpose + forward/loss/backward in one kernel + finalize
	STAGE_GRID_BWD_SCATTER,     // bucketed backward pass A: derive the corner records once, bin them by owning slice
	STAGE_GRID_BWD,             // pass B (owners accumulate + store, overflow records included) -- or the whole backward in the sliced / atomic modes
	STAGE_ADAM,
	// the direct exchange's phases (direct_exchange.h); recorded whenever a profiler is on, whatever `only_stage` says: they exist on N > 1 only,
	// where a step is long and the first node run has to explain itself
	STAGE_DX_WAIT_GRADS,   // signal "my gradients are final" + wait for every peer's
	STAGE_DX_REDUCE,       // read the peers' shards over the links, fp32 sum, one rounding
	STAGE_DX_PUSH,         // write the stepped shard into every peer's parameter buffer
	STAGE_DX_WAIT_PARAMS,  // signal "pushed" + wait for every peer's push
	N_STAGES
};
static const char* const STAGE_NAMES[N_STAGES] = {"grid_forward", "mlp_forward", "loss", "mlp_backward", "mlp_train_fused", "grid_backward_scatter", "grid_backward", "adam",
                                                  "exchange_wait_gradients", "exchange_reduce", "exchange_push", "exchange_wait_parameters"};

struct Profiler {
	int only_stage = -1;  // -1: all stages
	std::vector<hipEvent_t> pool;
	size_t next = 0;
	struct Span {
		int stage;
		hipEvent_t a, b;
		bool counts;
	};
	std::vector<Span> spans;
	double total_ms[N_STAGES] = {};
	uint64_t count[N_STAGES] = {};

	hipEvent_t get() {
		if (next == pool.size()) {
			hipEvent_t e;
			HIP_CHECK(hipEventCreate(&e));
			pool.push_back(e);
		}
		return pool[next++];
	}
	void collect() {
		for (auto& s : spans) {
			HIP_CHECK(hipEventSynchronize(s.b));
			float ms = 0.0f;
			HIP_CHECK(hipEventElapsedTime(&ms, s.a, s.b));
			total_ms[s.stage] += ms;
			if (s.counts) count[s.stage]++;
		}
		spans.clear();
		next = 0;
	}
	~Profiler() {
		for (auto e : pool) (void)hipEventDestroy(e);
	}
};

// Times one stage on `stream` from construction to destruction.  `profiler` null: off (modules have none).
struct ProfScope {
	Profiler* profiler;
	hipStream_t stream;
	int stage;
	bool counts;  // false: a further piece of a stage that is launched in several parts per step (time adds up, the launch count does not)
	hipEvent_t a = nullptr;
	// any_stage: timed whatever the profiler's stage filter says (the direct exchange's Adam is one of the exchange's phases)
	ProfScope(Profiler* p, hipStream_t s, int st, bool counts_ = true, bool any_stage = false) : profiler(p), stream(s), stage(st), counts(counts_) {
		if (p && (p->only_stage < 0 || p->only_stage == st || st >= STAGE_DX_WAIT_GRADS || any_stage)) {
			a = p->get();
			HIP_CHECK(hipEventRecord(a, stream));
		}
	}
	~ProfScope() {
		if (a) {
			hipEvent_t b = profiler->get();
			(void)hipEventRecord(b, stream);
			profiler->spans.push_back({stage, a, b, counts});
		}
	}
};

}  // namespace tcnn_hip

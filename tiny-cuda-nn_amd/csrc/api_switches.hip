// api_switches.hip -- C ABI: the free functions (device, memory, logging, last error, random numbers) and the process-wide A/B
// switches, with their state in one place.
#include <atomic>
#include <cstdlib>
#include <string>

#include "device_alloc.h"
#include "elementwise_kernels.h"
#include "grid_kernels.h"
#include "host_common.h"
#include "scratch_cache.h"
#include "switches.h"

namespace tcnn_hip {

// ------------------------------------------------------------------------------------------------
// logging (common_host.h:46-69) and error state
// ------------------------------------------------------------------------------------------------
static void (*g_log_callback)(int, const char*) = nullptr;
static thread_local std::string g_last_error;  // the library's one thread_local: tcnn_last_error() is per calling thread by contract
void set_last_error(const std::string& msg) { g_last_error = msg; }

void log_message(int severity, const std::string& msg) {
	if (g_log_callback) {
		g_log_callback(severity, msg.c_str());
	} else if (severity == TCNN_LOG_WARNING || severity == TCNN_LOG_ERROR) {
		fprintf(stderr, "tiny-cuda-nn_amd %s: %s\n", severity == TCNN_LOG_WARNING ? "warning" : "error", msg.c_str());
	}
}

// the switches of switches.h
static int initial_grid_backward_mode() {
	const char* e = getenv("TCNN_GRID_BACKWARD");
	if (e && std::string(e) == "atomic") return (int)GridBackwardMode::Atomic;
	if (e && std::string(e) == "sliced_f32") return (int)GridBackwardMode::SlicedF32;
	if (e && std::string(e) == "sliced_f16") return (int)GridBackwardMode::SlicedF16;
	return (int)GridBackwardMode::Bucketed;  // default: derive each corner once, bin by owner, exact fixed-point accumulation
}
std::atomic<int> g_grid_backward_mode{initial_grid_backward_mode()};
std::atomic<int> g_fused_network_passes{1};
std::atomic<int> g_fused_identity_input{1};
std::atomic<int> g_finalize_in_optimizer{1};
std::atomic<int> g_fp32_second_order{0};

}  // namespace tcnn_hip

using namespace tcnn_hip;

extern "C" {

const char* tcnn_last_error(void) { return g_last_error.c_str(); }
uint32_t tcnn_batch_size_granularity(void) { return BATCH_SIZE_GRANULARITY; }
int tcnn_hip_device(void) {
	int d = -1;
	(void)hipGetDevice(&d);
	return d;
}
int tcnn_set_hip_device(int device) {
	TCNN_API_BEGIN
	HIP_CHECK(hipSetDevice(device));
	TCNN_API_END
}
void tcnn_free_temporary_memory(void) {
	ScratchCache::free_all();
	ZeroedCounters::free_all();
}
int tcnn_device_malloc(size_t bytes, void** out) {
	TCNN_API_BEGIN
	*out = device_malloc(bytes);
	TCNN_API_END
}
void tcnn_device_free(void* ptr) { device_free(ptr); }
int tcnn_debug_alloc_mode(void) { return (int)debug_alloc_mode(); }
int tcnn_debug_check_allocations(void) {
	if (debug_alloc_mode() == DebugAlloc::Off) return 0;
	std::string report;
	const size_t bad = DebugAllocator::get().check_all(&report);
	set_last_error(report);
	if (bad) log_message(TCNN_LOG_ERROR, "debug allocator: " + report);
	return (int)bad;
}
int tcnn_set_debug_launches(int enable) {
	debug_launch_flags() = (debug_launch_flags() & ~1) | (enable ? 1 : 0);
	return TCNN_OK;
}
int tcnn_has_networks(void) { return 1; }
// the loss scale is kept at 128 for bfloat16 as well: harmless for its range, and the exact fixed-point accumulation of
// the grid backward (2^-24 resolution) relies on gradients of that magnitude
float tcnn_default_loss_scale(int precision) { return precision == TCNN_PRECISION_FP32 ? 1.0f : LOSS_SCALE_FP16; }
int tcnn_preferred_precision(void) { return NATIVE_PRECISION; }
int tcnn_supports_jit_fusion(int) { return 0; }
void tcnn_set_log_callback(void (*callback)(int, const char*)) { g_log_callback = callback; }

int tcnn_generate_random_uniform(tcnn_stream_t stream, uint64_t seed, uint64_t* position, size_t n, float* out, float lower, float upper) {
	TCNN_API_BEGIN
	Pcg32 rng{seed};
	if (position && *position) rng.advance((int64_t)*position);
	generate_random_uniform((hipStream_t)stream, rng, n, out, lower, upper);
	if (position) *position += n;
	TCNN_API_END
}

int tcnn_generate_sinusoid_targets(tcnn_stream_t stream, uint32_t n, uint32_t n_input_dims, uint32_t n_output_dims, const float* positions, float* targets) {
	TCNN_API_BEGIN
	if (n_input_dims == 0) throw std::runtime_error("tcnn_generate_sinusoid_targets: n_input_dims must be positive");
	if ((uint64_t)n * n_output_dims > 0xFFFFFFFFull) throw std::runtime_error("tcnn_generate_sinusoid_targets: batch too large");
	sinusoid_targets((hipStream_t)stream, n, n_input_dims, n_output_dims, positions, targets);
	TCNN_API_END
}

// The stream-ordered arena of the reference (GPUMemoryArena, gpu_memory.h:405-700; allocate_workspace(stream, bytes)) as the host
// sees it: a block out of the library's stream-keyed cache -- what the library's own scratch memory comes from -- handed back to the
// cache, not to the driver, when the host is done with it.  A block released on a stream is reused by later requests ON THAT STREAM
// only (work queued there is ordered behind its previous user); *granted is what to pass back.
int tcnn_stream_malloc(tcnn_stream_t stream, size_t bytes, void** out, size_t* granted) {
	TCNN_API_BEGIN
	if (!out || !granted) throw std::runtime_error("tcnn_stream_malloc: missing output argument");
	*out = ScratchCache::acquire((hipStream_t)stream, bytes, granted);
	TCNN_API_END
}
int tcnn_stream_free(tcnn_stream_t stream, void* ptr, size_t granted) {
	TCNN_API_BEGIN
	if (ptr) ScratchCache::release(stream_key((hipStream_t)stream), ptr, granted);
	TCNN_API_END
}

int tcnn_set_fused_identity_input(int enable) {
	g_fused_identity_input.store(enable != 0 ? 1 : 0);
	return TCNN_OK;
}
int tcnn_set_finalize_in_optimizer(int enable) {
	g_finalize_in_optimizer.store(enable != 0 ? 1 : 0);
	return TCNN_OK;
}
int tcnn_get_fused_network_passes(void) { return g_fused_network_passes.load(); }

int tcnn_set_fused_network_passes(int enable) {
	g_fused_network_passes.store(enable != 0 ? 1 : 0);
	return TCNN_OK;
}
int tcnn_grid_owner_wide_slices(uint64_t* out) {
	TCNN_API_BEGIN
	*out = grid_owner_wide_slices();
	TCNN_API_END
}
int tcnn_get_grid_owner_mode(void) { return grid_owner_mode(); }
int tcnn_set_grid_owner_mode(int mode) {
	if (mode < 0 || mode > 2) return TCNN_ERROR;
	grid_owner_mode() = mode;
	return TCNN_OK;
}
int tcnn_get_grid_backward_mode(void) { return g_grid_backward_mode.load(); }
int tcnn_set_grid_backward_mode(int mode) {
	if (mode < 0 || mode > 3) return TCNN_ERROR;
	g_grid_backward_mode.store(mode);
	return TCNN_OK;
}
int tcnn_get_fp32_second_order(void) { return g_fp32_second_order.load(); }
int tcnn_set_fp32_second_order(int mode) {
	if (mode < 0 || mode > 1) return TCNN_ERROR;
	g_fp32_second_order.store(mode);
	return TCNN_OK;
}

}  // extern "C"

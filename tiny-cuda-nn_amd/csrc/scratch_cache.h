// scratch_cache.h -- temporary device memory of the host layer, recycled per (device, stream).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace tcnn_hip {

// ------------------------------------------------------------------------------------------------
// (device, stream)-keyed scratch cache (stands where the reference's per-stream GPUMemoryArena stands,
// gpu_memory.h:405-700; its null-stream arenas are per device, global_gpu_memory_arenas()[cuda_device()]): blocks are
// recycled per stream of one device, so steady-state steps allocate nothing (a precondition for hipGraph capture), a
// recycled block is only ever reused in stream order, and a block never crosses to another GPU (the default stream's
// handle is 0 on every device).
// ------------------------------------------------------------------------------------------------
typedef std::pair<int, hipStream_t> StreamKey;
StreamKey stream_key(hipStream_t stream);

class ScratchCache {
public:
	static void* acquire(hipStream_t stream, size_t bytes, size_t* granted);
	static void release(const StreamKey& key, void* p, size_t bytes);
	static void free_all();
};

// Small per-stream device buffers that are zero whenever no kernel of that stream is using them (the bucketed grid
// backward's queue counters: its kernels hand them back zeroed, so they are cleared exactly once, at allocation).
class ZeroedCounters {
public:
	static uint32_t* get(hipStream_t stream, size_t n);
	static void free_all();
};

// one block out of the cache, owned until the object goes (then back to its stream's list)
struct Scratch {
	void* ptr = nullptr;
	size_t bytes = 0;
	StreamKey stream = {0, nullptr};  // (device, stream) the block belongs to
	Scratch() = default;
	Scratch(hipStream_t s, size_t n_bytes) : stream(stream_key(s)) { ptr = ScratchCache::acquire(s, n_bytes, &bytes); }
	Scratch(const Scratch&) = delete;
	Scratch& operator=(const Scratch&) = delete;
	Scratch(Scratch&& o) noexcept { *this = std::move(o); }
	Scratch& operator=(Scratch&& o) noexcept {
		reset();
		ptr = o.ptr;
		bytes = o.bytes;
		stream = o.stream;
		o.ptr = nullptr;
		return *this;
	}
	~Scratch() { reset(); }
	void reset() {
		if (ptr) ScratchCache::release(stream, ptr, bytes);
		ptr = nullptr;
	}
	template <typename T>
	T* as() const { return (T*)ptr; }
};

}  // namespace tcnn_hip

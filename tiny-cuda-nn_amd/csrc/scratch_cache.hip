// scratch_cache.hip -- the (device, stream)-keyed block cache and zeroed counter buffers behind scratch_cache.h.
#include "scratch_cache.h"

#include <algorithm>
#include <map>
#include <mutex>

#include "device_alloc.h"
#include "host_common.h"

namespace tcnn_hip {

StreamKey stream_key(hipStream_t stream) {
	int device = 0;
	(void)hipGetDevice(&device);
	return {device, stream};
}

// process-wide state per (device, stream), behind one mutex
template <typename V>
struct PerStream {
	std::mutex mutex;
	std::map<StreamKey, V> map;
	// hands every entry to `free_entry` with its own device current and idle, then forgets them all
	template <typename F>
	void free_all(F free_entry) {
		std::lock_guard<std::mutex> lock(mutex);
		int before = 0;
		(void)hipGetDevice(&before);
		for (auto& kv : map) {
			(void)hipSetDevice(kv.first.first);
			(void)hipDeviceSynchronize();
			free_entry(kv.second);
		}
		(void)hipSetDevice(before);
		map.clear();
	}
};
static PerStream<std::multimap<size_t, void*>>& free_lists() {  // recycled blocks by size
	static PerStream<std::multimap<size_t, void*>> l;
	return l;
}
static PerStream<std::pair<uint32_t*, size_t>>& counter_slots() {  // (buffer, capacity in counters)
	static PerStream<std::pair<uint32_t*, size_t>> s;
	return s;
}

void* ScratchCache::acquire(hipStream_t stream, size_t bytes, size_t* granted) {
	const bool debug = debug_alloc_mode() != DebugAlloc::Off;
	// checking allocator (device_alloc.h): exact sizes, so that a block ends where the request ends, and fresh poison on
	// every hand-out, so that nothing can rely on what an earlier use left in a recycled block
	bytes = debug ? (bytes ? bytes : (size_t)1) : next_multiple(bytes ? bytes : (size_t)1, (size_t)256);
	{
		std::lock_guard<std::mutex> lock(free_lists().mutex);
		auto& fl = free_lists().map[stream_key(stream)];
		auto it = fl.lower_bound(bytes);
		if (it != fl.end() && it->first <= (debug ? bytes : 2 * bytes)) {
			void* p = it->second;
			*granted = it->first;
			fl.erase(it);
			if (debug) HIP_CHECK(hipMemsetAsync(p, DEBUG_POISON_BYTE, bytes, stream));
			return p;
		}
	}
	void* p = device_malloc(bytes);
	*granted = bytes;
	return p;
}
void ScratchCache::release(const StreamKey& key, void* p, size_t bytes) {
	std::lock_guard<std::mutex> lock(free_lists().mutex);
	free_lists().map[key].emplace(bytes, p);
}
void ScratchCache::free_all() {
	free_lists().free_all([](const std::multimap<size_t, void*>& blocks) {
		for (auto& b : blocks) device_free(b.second);
	});
}

uint32_t* ZeroedCounters::get(hipStream_t stream, size_t n) {
	std::lock_guard<std::mutex> lock(counter_slots().mutex);
	auto& slot = counter_slots().map[stream_key(stream)];
	if (slot.second < n) {
		if (slot.first) {
			HIP_CHECK(hipStreamSynchronize(stream));
			device_free(slot.first);
			slot = {nullptr, 0};
		}
		const size_t cap = std::max<size_t>(next_multiple<size_t>(n, 1024), 4096);
		void* p = device_malloc(cap * sizeof(uint32_t));
		HIP_CHECK(hipMemset(p, 0, cap * sizeof(uint32_t)));
		HIP_CHECK(hipDeviceSynchronize());
		slot = {(uint32_t*)p, cap};
	}
	return slot.first;
}
void ZeroedCounters::free_all() {
	counter_slots().free_all([](const std::pair<uint32_t*, size_t>& slot) { device_free(slot.first); });
}

}  // namespace tcnn_hip

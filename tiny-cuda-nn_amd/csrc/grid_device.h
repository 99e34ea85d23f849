// grid_device.h -- what every pass of the grid encoding shares: the level / cell arithmetic (bit-exact against the CPU oracle: build with
// -ffp-contract=off, the fp32 position / weight arithmetic must round exactly as written), the one statement of each per-level fact, and the
// D x F dispatch of the launchers.  See grid_kernels.h for the API and the reference lines restated.
//
// Input domain: positions need not lie in [0, 1).  Any finite x with |x| * scale + 0.5 < 2^31 at every level behaves as the reference's
// pos_fract does (common_device.h:1016-1043): cell coordinates wrap modulo 2^32 (cell -1 is 0xFFFFFFFF), are hashed or taken modulo the table
// size, and the weights come from the fraction; nothing is clamped, and every shortcut on top of make_cell (hhi = hlo + prime, the pair tag of
// the record scatter, the dense i1 = i0 + 1) holds for wrapped cells (tests/grid_domain_positions.py, tests/test_emu_grid_domain.py).  NaN, Inf
// and larger magnitudes are unspecified, as in the reference: its float -> int conversion is undefined there.
#pragma once
#include "grid_kernels.h"

#include <stdexcept>
#include <type_traits>

namespace tcnn_hip {

constexpr uint32_t GRID_THREADS = 256;
constexpr uint32_t GRID_SPT = 4;  // samples per thread (independent gathers in flight per lane)
constexpr uint32_t GRID_TILE = GRID_THREADS * GRID_SPT;

// Work distribution: block b -> (level, tile) with level % 8 == b % 8.  Blocks are dispatched
// round-robin over the 8 XCDs (observed, not guaranteed): every XCD then gathers from ceil(L/8)
// level tables only, in level order, so one table at a time is hot in its private L2
// (measured: 237 G gathers/s with XCD-local tables vs 67 G/s mixed, profiles/r01_microbench_atomics.txt).
TCNN_DEVICE bool grid_work_item(uint32_t n_levels, uint32_t tiles, uint32_t& level, uint32_t& tile) {
	const uint32_t b = blockIdx.x, xcd = b & 7u, slot = b >> 3;
	if (xcd >= n_levels) return false;
	const uint32_t levels_here = (n_levels - xcd + 7u) / 8u;
	if (slot >= levels_here * tiles) return false;
	level = xcd + 8u * (slot / tiles);
	tile = slot % tiles;
	return true;
}

static inline uint32_t grid_n_blocks(uint32_t n_levels, uint32_t n) {
	return 8u * div_round_up(n_levels, 8u) * div_round_up(n, GRID_TILE);
}

// ---------------------------------------------------------------------------------------------
// per-level constants and per-sample cell data shared by every kernel below
// ---------------------------------------------------------------------------------------------
template <uint32_t D>
struct Level {
	uint32_t hashmap_size, resolution, mask;
	float scale;
	bool is_hash, smooth, nearest;
	bool fast;  // hashed level with a power-of-two table: index = coherent_prime_hash & mask
};

// Table geometry of one level -- grid_index's decision (common_device.h:868-881), stated once for the kernels and the host planners: a
// level is hashed iff its table is smaller than the dense grid, resolution^D entries.  `dense` is that product while it fits 32 bits
// (resolution <= MAX_BASES[D]) and 0xFFFFFFFF, "beyond 32 bits", otherwise: no table has that many entries (level sizes are multiples
// of 8), so every comparison against it comes out as it would against the true product.
struct LevelGeometry {
	uint32_t entries, dense;
	bool hashed;  // indexed by coherent_prime_hash, not densely
	bool fast;    // hashed with a power-of-two table: index = hash & mask
};
template <uint32_t D>
TCNN_HOST_DEVICE LevelGeometry level_geometry(const GridMeta& meta, uint32_t level) {
	constexpr uint32_t MAX_BASES[11] = {0x0, 0xFFFFFFFF, 0xFFFF, 0x659, 0xFF, 0x54, 0x28, 0x17, 0xF, 0xB, 0x9};
	LevelGeometry geo;
	geo.entries = meta.offset[level + 1] - meta.offset[level];
	const uint32_t resolution = meta.resolution[level];
	geo.dense = 0xFFFFFFFFu;
	if (resolution <= MAX_BASES[D]) {
		geo.dense = 1;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) geo.dense *= resolution;
	}
	const bool is_hash = meta.grid_type == (uint32_t)GridType::Hash;
	geo.hashed = is_hash && geo.entries < geo.dense;
	geo.fast = is_hash && geo.entries < geo.dense && (geo.entries & (geo.entries - 1u)) == 0u;
	return geo;
}
// the same for the host planners, by the encoding's own number of dimensions
inline LevelGeometry level_geometry(const GridMeta& meta, uint32_t level) {
	switch (meta.n_dims) {
		case 2: return level_geometry<2>(meta, level);
		case 3: return level_geometry<3>(meta, level);
		case 4: return level_geometry<4>(meta, level);
		default: throw std::runtime_error("GridEncoding: number of input dims must be 2, 3 or 4.");
	}
}

template <uint32_t D>
TCNN_DEVICE Level<D> make_level(const GridMeta& meta, uint32_t level) {
	Level<D> lv;
	lv.hashmap_size = meta.offset[level + 1] - meta.offset[level];
	lv.resolution = meta.resolution[level];
	lv.mask = lv.hashmap_size - 1u;
	lv.scale = meta.scale[level];
	lv.is_hash = meta.grid_type == (uint32_t)GridType::Hash;
	lv.smooth = meta.interp == (uint32_t)InterpolationType::Smoothstep;
	lv.nearest = meta.interp == (uint32_t)InterpolationType::Nearest;
	lv.fast = level_geometry<D>(meta, level).fast;
	return lv;
}

TCNN_DEVICE float smoothstep(float v) { return v * v * (3.0f - 2.0f * v); }
TCNN_DEVICE float smoothstep_derivative(float v) { return 6 * v * (1.0f - v); }

template <uint32_t D>
struct Cell {
	uint32_t grid[D];         // integer cell coordinate (may wrap, common_device.h:1002-1007)
	uint32_t hlo[D], hhi[D];  // grid[d] * prime[d] and (grid[d] + 1) * prime[d]  (mod 2^32)
	float w[D][2];            // [d][0] = 1 - frac, [d][1] = frac  (after the interpolation function)
	float derivative[D];
};

// reference common_device.h:1016-1043 (pos_fract) for every dimension of one sample (x = its position)
// NOT_SMOOTH: the caller has established that the level does not interpolate with Smoothstep (the record scatter decides it once per
// workgroup): the run-time form computes both and selects per value
template <uint32_t D, bool FAST, bool NOT_SMOOTH = false>
TCNN_DEVICE Cell<D> make_cell(const Level<D>& lv, const float (&x)[D]) {
	constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
	Cell<D> c;
	const bool smooth = NOT_SMOOTH ? false : lv.smooth;
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		float p = __builtin_fmaf(lv.scale, x[d], 0.5f);
		const float tmp = __builtin_floorf(p);
		c.grid[d] = (uint32_t)(int)tmp;
		p -= tmp;
		c.derivative[d] = smooth ? smoothstep_derivative(p) : 1.0f;
		if (smooth) p = smoothstep(p);
		c.w[d][0] = 1 - p;
		c.w[d][1] = p;
		if constexpr (FAST) {
			c.hlo[d] = c.grid[d] * primes[d];
			c.hhi[d] = c.hlo[d] + primes[d];
		}
	}
	return c;
}

template <uint32_t D, bool TRY_PACKED = false>
TCNN_DEVICE void load_position(const GridIO& io, uint32_t i, float (&x)[D]) {
#if !defined(TCNN_HOST_EMU)
	// (forward kernels only: in the record scatter the same load measured 8 us SLOWER than three strided dword loads)
	if (TRY_PACKED && io.pos_stride_d == 1u && io.pos_stride_i == D) {
		// sample-major contiguous positions (what every caller of the hot path passes): ONE D-dword load per lane instead of D
		// strided ones (a 12-byte lane stride costs an instruction ~20 clk whatever its width; wave-uniform branch).  A buffer
		// load, because the 4-byte-aligned 12-byte access is split into two by the compiler in its global form.
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)io.positions, 0, (int)(io.n * D * 4u), 0x00020000);
		// (the result is cast as a whole: indexing the builtin's vector_size type directly is miscompiled by ROCm 7.2's clang into
		// one dword splat over all elements; the 16-byte form is narrowed to the 12 bytes that are used)
		typedef float f2 __attribute__((ext_vector_type(2)));
		if constexpr (D == 2) {
			const f2 p = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(i * D * 4u), 0, 0));
			x[0] = p[0];
			x[1] = p[1];
		} else {
			const f4 p = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(i * D * 4u), 0, 0));
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) x[d] = p[d];
		}
		return;
	}
#endif
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = io.positions[(size_t)i * io.pos_stride_i + (size_t)d * io.pos_stride_d];
}

template <uint32_t D, bool FAST>
TCNN_DEVICE Cell<D> make_cell(const Level<D>& lv, const GridIO& io, uint32_t i) {
	float x[D];
	load_position<D>(io, i, x);
	return make_cell<D, FAST>(lv, x);
}

// entry index of corner `idx` (bit d of idx selects +1 in dimension d, grid.h:147-160)
template <uint32_t D, bool FAST>
TCNN_DEVICE uint32_t corner_index(const Level<D>& lv, const Cell<D>& c, uint32_t idx) {
	if constexpr (FAST) {
		uint32_t h = 0;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) h ^= ((idx >> d) & 1u) ? c.hhi[d] : c.hlo[d];
		return h & lv.mask;
	} else {
		uint32_t local[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) local[d] = c.grid[d] + ((idx >> d) & 1u);
		return grid_index<D>(lv.is_hash, lv.hashmap_size, lv.resolution, local);
	}
}

// interpolation weight of corner `idx`: ((1 * w0) * w1) * w2 ... in the reference's order (grid.h:148-160)
template <uint32_t D>
TCNN_DEVICE float corner_weight(const Cell<D>& c, uint32_t idx) {
	float weight = ((idx & 1u) ? c.w[0][1] : c.w[0][0]);
#pragma unroll
	for (uint32_t d = 1; d < D; ++d) weight *= ((idx >> d) & 1u) ? c.w[d][1] : c.w[d][0];
	return weight;
}

// Corner weight of the SECOND-ORDER scatter (kernel_grid_backward_input_backward_grid, grid.h:427-455, summed over the
// gradient dimensions): scale * sum_d ddx[d] * pos'(d) * (+1 right / -1 left along d) * prod_{e != d} w_e(corner).
template <uint32_t D>
TCNN_DEVICE float corner_weight_second_order(const Level<D>& lv, const Cell<D>& c, uint32_t idx, const float (&ddx)[D]) {
	float total = 0.0f;
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		float weight = lv.scale * ddx[d] * c.derivative[d];
#pragma unroll
		for (uint32_t e = 0; e < D; ++e) {
			if (e != d) weight *= ((idx >> e) & 1u) ? c.w[e][1] : c.w[e][0];
		}
		total += ((idx >> d) & 1u) ? weight : -weight;
	}
	return total;
}
// fp32 encodings, second order: Smoothstep's lower weight as S(1 - t), which equals 1 - S(t).  make_cell's 1 - S(t) (the reference's form,
// kept where results are held bit for bit) subtracts a ROUNDED S(t) and loses its relative accuracy as t -> 1; 1 - t is one rounding of the
// exact fraction and S of it carries a few more, whatever its size.  Linear's 1 - t is left as it is.
template <uint32_t D>
TCNN_DEVICE void second_order_weights_f32(const Level<D>& lv, const float (&x)[D], Cell<D>& c) {
	if (!lv.smooth) return;
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		float p = __builtin_fmaf(lv.scale, x[d], 0.5f);
		p -= __builtin_floorf(p);
		c.w[d][0] = smoothstep(1.0f - p);
	}
}
template <uint32_t D>
TCNN_DEVICE void load_ddx(const GridIO& io, uint32_t i, float (&v)[D]) {
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) v[d] = io.ddx[(size_t)i * io.ddx_stride_i + (size_t)d * io.ddx_stride_d];
}

// F halves at `p` -> NP packed pairs (F == 1: {x, 0})
template <uint32_t F>
TCNN_DEVICE void load_features(const half_t* p, h2 (&v)[(F + 1) / 2]) {
	if constexpr (F == 1) {
		v[0] = h2{p[0], (half_t)0.0f};
	} else if constexpr (F == 2) {
		v[0] = *(const h2*)p;
	} else if constexpr (F == 4) {
		const h4 t = *(const h4*)p;
		v[0] = h2{t[0], t[1]};
		v[1] = h2{t[2], t[3]};
	} else {
		static_assert(F == 8, "n_features_per_level must be 1, 2, 4 or 8 (grid.h:1811-1821)");
		const h8 t = *(const h8*)p;
		v[0] = h2{t[0], t[1]};
		v[1] = h2{t[2], t[3]};
		v[2] = h2{t[4], t[5]};
		v[3] = h2{t[6], t[7]};
	}
}

// F floats at `p` (an fp32 table: entries are F * 4 bytes apart, so the entry's own alignment holds) -> v; one 8-byte load at F == 2, 16-byte
// loads from F == 4 on
template <uint32_t F>
TCNN_DEVICE void load_features(const float* p, float (&v)[F]) {
	if constexpr (F == 1) {
		v[0] = p[0];
	} else if constexpr (F == 2) {
		const f2 t = *(const f2*)p;
		v[0] = t[0];
		v[1] = t[1];
	} else {
		static_assert(F == 4 || F == 8, "n_features_per_level must be 1, 2, 4 or 8 (grid.h:1811-1821)");
#pragma unroll
		for (uint32_t q = 0; q < F / 4; ++q) {
			const f4 t = *(const f4*)(p + 4 * q);
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) v[4 * q + j] = t[j];
		}
	}
}

// Is `level` switched off by max_level (MultiLevelEncoding::m_max_level)?  The reference tests '>=' in the forward pass (grid.h:75,
// INCLUSIVE) and '>' in the backward passes (grid.h:242, 483) -- sic, both are restated; the float expression is grid.h:72's, as written.
template <bool INCLUSIVE>
TCNN_HOST_DEVICE bool level_is_off(const GridMeta& meta, float max_level_value, uint32_t level, uint32_t F) {
	const uint32_t n_features = meta.n_levels * F;
	const float max_level = (max_level_value * (float)n_features) / (float)F;
	return INCLUSIVE ? (float)level >= max_level + 1e-3f : (float)level > max_level + 1e-3f;
}
template <bool INCLUSIVE>
TCNN_HOST_DEVICE bool level_is_off(const GridMeta& meta, uint32_t level, uint32_t F) {
	return level_is_off<INCLUSIVE>(meta, meta.max_level, level, F);
}
// The per-sample form (set_max_level_gpu, grid.h:70-72: the array wins over the scalar): is `level` off for sample i?  Only where
// io.max_level is set -- the kernels test that pointer once, wave-uniformly, and keep the scalar's per-level answer otherwise.
template <bool INCLUSIVE>
TCNN_DEVICE bool level_is_off(const GridMeta& meta, const GridIO& io, uint32_t i, uint32_t level, uint32_t F) {
	return level_is_off<INCLUSIVE>(meta, io.max_level[i], level, F);
}

// Calls fn(D, F), two std::integral_constants, for the encoding's dimensions and features per level: every launcher instantiates its
// kernels for the same 3 x 4 combinations.
template <typename FN>
static inline void grid_dispatch(const GridMeta& meta, FN&& fn) {
	auto with_d = [&](auto d) {
		switch (meta.n_feat) {
			case 1: fn(d, std::integral_constant<uint32_t, 1>{}); break;
			case 2: fn(d, std::integral_constant<uint32_t, 2>{}); break;
			case 4: fn(d, std::integral_constant<uint32_t, 4>{}); break;
			case 8: fn(d, std::integral_constant<uint32_t, 8>{}); break;
			default: throw std::runtime_error("GridEncoding: n_features_per_level must be 1, 2, 4, or 8.");
		}
	};
	switch (meta.n_dims) {
		case 2: with_d(std::integral_constant<uint32_t, 2>{}); break;
		case 3: with_d(std::integral_constant<uint32_t, 3>{}); break;
		case 4: with_d(std::integral_constant<uint32_t, 4>{}); break;
		default: throw std::runtime_error("GridEncoding: number of input dims must be 2, 3 or 4.");
	}
}

}  // namespace tcnn_hip

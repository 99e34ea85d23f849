// mlp_general_f32.hip -- the layer-by-layer network with fp32 weights, activations and gradients (mlp_general_f32.h).  The structure of
// mlp_general.hip with float where it has the 16-bit type and v_mfma_f32_16x16x4_f32 where it has v_mfma_f32_16x16x32_f16:
//   * k_mlp_f32_layer:  Y[sample][m] = epilogue(sum_k Wm[m][k] X[sample][k]) for one matrix Wm [M][K] row-major.  Forward: Wm = a layer's
//     weights, epilogue = activation (SiLU / Sine in a training pass: the accumulator is stored as the pre-activation as well).  Backward:
//     Wm = the transposed weights, X = dL/d(pre-activation) of the layer above, epilogue = the derivative at the saved post-activation
//     (SiLU / Sine: pre-activation) values.  Nothing is rounded between the accumulator and the store.
//     The 16x16x4 shape: lane (lr = lane & 15, g = lane >> 4) supplies ONE float per operand, A[i = lr][k = g] and B[k = g][n = lr], and the
//     C/D fragment is that of the 16-bit shapes (row = 4 g + r, col = lr).  Weights are the A operand, activations the B operand, so the
//     accumulator fragment is 4 consecutive m of one sample: a 16-byte store into the sample-major result, as in mlp_general.hip.  Which k a
//     lane's operand element stands for is free as long as A and B agree: a lane reads 4 consecutive k of its row with ONE 16-byte LDS read
//     per operand block (k = 16 kk + 4 g + j) and feeds element j to the j-th of four MFMAs.
//     Workgroup: 4 waves, tile = (16 * NMB m) x (128 samples); wave w owns samples 32 w .. 32 w + 31 and all NMB blocks of m
//     (2 B reads + NMB A reads per 8 * NMB MFMAs; 2 * NMB independent accumulators cover the shape's 40-cycle dependent latency).  K runs in
//     steps of 32 through two LDS stages -- the global loads of step s + 1 are all issued into registers before the MFMAs of step s and
//     written to the other stage after them (every load of a strip before its first store), one barrier per step.  Rows of 32 + 4 floats
//     (144 bytes, the byte stride of mlp_general.hip's rows): the 16 rows of a 16-byte fragment read start 36 banks apart -- conflict-free.
//     LDS: 2 * (64 + 128) * 144 B = 54 KiB at NMB = 4, whatever the network's width (a width of 1024 is 16 m tiles and 32 K steps).
//   * k_mlp_f32_wgrad:  dW[o][i] = sum_s d[s][o] a[s][i] for one 64 x 64 tile of one matrix over one slice of the batch.  Both operands
//     arrive sample-major and are staged as they lie with 16-byte copies; with one float per lane and operand the "samples in k" fragment
//     is a plain 4-byte LDS read of row 4 q + g, column lr (no transpose read): rows of 64 + 16 floats put the four rows of a read 16 banks
//     apart -- conflict-free.  The feature-major network input is staged [feature][sample] in rows of 32 + 4 floats.  32 samples per stage,
//     two stages (40 KiB).  The batch is cut into mlp_f32_n_partials slices; slice s writes its tiles into slab s in parameter order and
//     k_mlp_f32_finalize sums the slabs in ascending order: deterministic, no floating-point atomics, independent of the launch geometry.
#include "mlp_general_f32.h"

#if !defined(TCNN_HOST_EMU)
#include "scratch_cache.h"
#endif

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace tcnn_hip {

#if !defined(TCNN_HOST_EMU)
// A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15]; D row = 4 (lane >> 4) + r, col = lane & 15.  A k-ordered fmaf chain.
TCNN_DEVICE f4 mfma_16x16x4_f32(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
#endif

constexpr uint32_t G32_THREADS = 256;
constexpr uint32_t G32_BN = 128;            // samples per workgroup tile of k_mlp_f32_layer
constexpr uint32_t G32_BK = 32;             // k per LDS stage
constexpr uint32_t G32_LDK = G32_BK + 4;    // row stride (floats) of the [row][k] stages
constexpr uint32_t G32_MAX_MB = 4;          // blocks of 16 m per workgroup tile, at most

// ---- activations on fp32 values (common_device.h:108-186 forward, :363-418 and :253-277 backward, with T = float).  ReLU / None stay
// inline as selects; everything else is ONE out-of-line body per kernel, entered once per fragment (activation_device.h says why).
TCNN_DEVICE_NOINLINE f4 act32_forward4_general(uint32_t act, f4 x) {
	f4 y;
	switch ((Activation)act) {
		case Activation::LeakyReLU:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] > 0.0f ? x[j] : x[j] * 0.01f;
			break;
		case Activation::Exponential:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = expf(x[j]);
			break;
		case Activation::Sigmoid:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = 1.0f / (1.0f + expf(-x[j]));
			break;
		case Activation::Squareplus:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) {
				const float t = x[j] * K_ACT;
				y[j] = 0.5f * (t + sqrtf(t * t + 4.0f)) / K_ACT;
			}
			break;
		case Activation::Softplus:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = logf(expf(x[j] * K_ACT) + 1.0f) / K_ACT;
			break;
		case Activation::Tanh:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = tanhf(x[j]);
			break;
		case Activation::SiLU:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] * (1.0f / (1.0f + expf(-x[j])));
			break;
		case Activation::Sine:  // the accurate sinf: first-layer pre-activations of a SIREN network are tens of radians
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = sinf(x[j]);
			break;
		case Activation::ReLU:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] > 0.0f ? x[j] : 0.0f;
			break;
		default: y = x; break;
	}
	return y;
}
template <bool GENERAL>
TCNN_DEVICE f4 act32_forward4(uint32_t act, f4 x) {
	if constexpr (GENERAL) {
		mfma_settle(x);  // the fragment is read on both sides of the branch below
		if (act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU) x = act32_forward4_general(act, x);
	}
	const bool relu = act == (uint32_t)Activation::ReLU;  // a select on a uniform flag, not a branch behind the MFMA (act_forward4)
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) x[j] = (relu && !(x[j] > 0.0f)) ? 0.0f : x[j];
	return x;
}
// v * f'(.) with f' through `aux`: the post-activation value, or -- SiLU / Sine -- the pre-activation
TCNN_DEVICE_NOINLINE f4 act32_backward4_general(uint32_t act, f4 v, f4 aux) {
	f4 out;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) {
		const float y = aux[j];
		float factor = 1.0f;
		switch ((Activation)act) {  // (uniform: hoisted out of the unrolled loop)
			case Activation::ReLU: factor = y > 0.0f ? 1.0f : 0.0f; break;
			case Activation::LeakyReLU: factor = y > 0.0f ? 1.0f : 0.01f; break;
			case Activation::Exponential: factor = y; break;
			case Activation::Sigmoid: factor = y * (1.0f - y); break;
			case Activation::Squareplus: {
				const float t = y * K_ACT;
				factor = t * t / (t * t + 1.0f);
				break;
			}
			case Activation::Softplus: factor = 1.0f - expf(-y * K_ACT); break;
			case Activation::Tanh: factor = 1.0f - y * y; break;
			case Activation::SiLU: {
				const float l = 1.0f / (1.0f + expf(-y));
				factor = l + y * (l * (1.0f - l));
				break;
			}
			case Activation::Sine: factor = cosf(y); break;
			default: break;
		}
		out[j] = v[j] * factor;
	}
	return out;
}
template <bool GENERAL>
TCNN_DEVICE f4 act32_backward4(uint32_t act, f4 v, f4 aux) {
	if constexpr (GENERAL) {
		mfma_settle(v);
		if (act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU) v = act32_backward4_general(act, v, aux);
	}
	const bool relu = act == (uint32_t)Activation::ReLU;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) v[j] = (relu && !(aux[j] > 0.0f)) ? 0.0f : v[j];
	return v;
}

// _TRIMMED: G32_EPI_FORWARD whose result goes to the caller's trimmed matrix (Yt ...) instead of Y
enum : uint32_t { G32_EPI_NONE = 0, G32_EPI_FORWARD = 1, G32_EPI_BACKWARD = 2, G32_EPI_FORWARD_TRIMMED = 3 };

struct Gen32LayerArgs {
	uint32_t n, M, K;
	const float* Wm;      // [M][K] row-major
	const float* X;       // sample-major [n][ldx], or feature-major [K][n] (X_FM)
	uint32_t ldx;
	float* Y;             // sample-major [n][ldy], or feature-major [M][n] (Y_FM)
	uint32_t ldy;
	const float* F;       // G32_EPI_BACKWARD: the values the derivative is taken at (post-activations; SiLU / Sine: pre-activations), [n][ldf]
	uint32_t ldf;
	uint32_t act;
	float* P;             // G32_EPI_FORWARD: where the pre-activations go, sample-major [n][ldy]; null: not saved
	// G32_EPI_FORWARD_TRIMMED: element (sample i, m) with m < t_dims at Yt[i * t_stride_i + m * t_stride_j].  t_vec: floats per store the
	// host proved aligned for EVERY (sample, m = multiple of 4) -- 4 or 2 only with t_stride_j == 1 (g32_trimmed_vec) -- else 1
	float* Yt;
	uint32_t t_dims, t_stride_i, t_stride_j, t_vec;
};

// the 4 values of one accumulator fragment (m .. m + 3 of one sample) into the caller's trimmed matrix.  Nothing at or past t_dims is written.
TCNN_DEVICE void g32_store_trimmed(const Gen32LayerArgs& a, size_t sample, uint32_t m, f4 v) {
	float* p = a.Yt + sample * a.t_stride_i + (size_t)m * a.t_stride_j;
	if (a.t_vec == 4u && m + 4u <= a.t_dims) {
		*(f4*)p = v;
	} else if (a.t_vec >= 2u) {
#pragma unroll
		for (uint32_t q = 0; q < 2; ++q) {
			if (m + 2u * q + 2u <= a.t_dims) {
				*(f2*)(p + 2u * q) = f2{v[2 * q], v[2 * q + 1]};
			} else if (m + 2u * q < a.t_dims) {
				p[2u * q] = v[2 * q];
			}
		}
	} else {
#pragma unroll
		for (uint32_t r = 0; r < 4; ++r)
			if (m + r < a.t_dims) p[(size_t)r * a.t_stride_j] = v[r];
	}
}

template <uint32_t NMB, uint32_t EPI, bool X_FM, bool Y_FM, bool GENERAL>
__global__ void __launch_bounds__(G32_THREADS) k_mlp_f32_layer(const Gen32LayerArgs a) {
	constexpr uint32_t BM = 16 * NMB, CK = G32_BK / 4;  // 16-byte chunks per row of a stage
	constexpr uint32_t W_CHUNKS = BM * CK, X_CHUNKS = G32_BN * CK;
	constexpr uint32_t W_PER = (W_CHUNKS + G32_THREADS - 1) / G32_THREADS, X_PER = X_CHUNKS / G32_THREADS;
	constexpr uint32_t STAGE = (BM + G32_BN) * G32_LDK;
	TCNN_DYN_LDS(lds_raw);
	float* lds = (float*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t n_mt = div_round_up(a.M, BM);
	const uint32_t m0 = (blockIdx.x % n_mt) * BM;  // m tiles fastest: neighbouring workgroups share their sample tile in L2
	const size_t s0 = (size_t)(blockIdx.x / n_mt) * G32_BN;
	const uint32_t n_steps = div_round_up(a.K, G32_BK);
	const f4 zero = zero4();

	// one K step of both operands, global -> registers.  Chunks past M or K read a valid address and are replaced by zeros (K is a
	// multiple of 16, a chunk is 4: wholly inside or outside) -- a select, not a branch around the load.
	f4 wreg[W_PER], xreg[X_PER];
	auto load = [&](uint32_t k0) {
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS, row = c / CK, kc = c % CK;
			const bool valid = c < W_CHUNKS && m0 + row < a.M && k0 + 4 * kc < a.K;
			const f4 v = *(const f4*)(a.Wm + (valid ? (size_t)(m0 + row) * a.K + k0 + 4 * kc : (size_t)0));
			wreg[q] = valid ? v : zero;
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS;
			if constexpr (X_FM) {  // consecutive lanes = consecutive features: the transposing 4-byte stores below fall into one row
				const uint32_t k = c % G32_BK, sc = c / G32_BK;
				const bool valid = k0 + k < a.K;
				const f4 v = *(const f4*)(a.X + (size_t)(valid ? k0 + k : 0u) * a.n + s0 + 4 * sc);
				xreg[q] = valid ? v : zero;
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				const bool valid = k0 + 4 * kc < a.K;
				const f4 v = *(const f4*)(a.X + (s0 + row) * a.ldx + (valid ? k0 + 4 * kc : 0u));
				xreg[q] = valid ? v : zero;
			}
		}
	};
	auto store = [&](float* stage) {
		float* Wt = stage;
		float* Xt = stage + BM * G32_LDK;
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS, row = c / CK, kc = c % CK;
			if (c < W_CHUNKS) *(f4*)(Wt + row * G32_LDK + 4 * kc) = wreg[q];
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS;
			if constexpr (X_FM) {
				const uint32_t k = c % G32_BK, sc = c / G32_BK;
#pragma unroll
				for (uint32_t j = 0; j < 4; ++j) Xt[(4 * sc + j) * G32_LDK + k] = xreg[q][j];
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				*(f4*)(Xt + row * G32_LDK + 4 * kc) = xreg[q];
			}
		}
	};

	f4 acc[NMB][2];
#pragma unroll
	for (uint32_t mb = 0; mb < NMB; ++mb) {
		acc[mb][0] = zero4();
		acc[mb][1] = zero4();
	}

	load(0);
	store(lds);
	__syncthreads();
	for (uint32_t ks = 0; ks < n_steps; ++ks) {
		const float* Wt = lds + (ks & 1u) * STAGE;
		const float* Xt = Wt + BM * G32_LDK;
		const bool more = ks + 1 < n_steps;
		if (more) load((ks + 1) * G32_BK);  // in flight while the MFMAs below run
#pragma unroll
		for (uint32_t kk = 0; kk < G32_BK / 16; ++kk) {
			f4 bv[2];
#pragma unroll
			for (uint32_t sb = 0; sb < 2; ++sb) bv[sb] = *(const f4*)(Xt + (32 * w + 16 * sb + lr) * G32_LDK + 16 * kk + 4 * g);
#pragma unroll
			for (uint32_t mb = 0; mb < NMB; ++mb) {
				const f4 av = *(const f4*)(Wt + (16 * mb + lr) * G32_LDK + 16 * kk + 4 * g);
#pragma unroll
				for (uint32_t j = 0; j < 4; ++j)
#pragma unroll
					for (uint32_t sb = 0; sb < 2; ++sb) acc[mb][sb] = mfma_16x16x4_f32(av[j], bv[sb][j], acc[mb][sb]);
			}
		}
		if (more) store(lds + ((ks + 1) & 1u) * STAGE);  // the stage every wave finished reading before the last barrier
		__syncthreads();
	}

	// accumulator element r <-> (m = m0 + 16 mb + 4 g + r, sample = s0 + 32 w + 16 sb + lr).  Blocks past M are computed and not stored; the
	// results are read behind the loop's exit and that branch, so the MFMA wait states are spent here (activation_device.h mfma_settle).
#pragma unroll
	for (uint32_t mb = 0; mb < NMB; ++mb) {
		mfma_settle(acc[mb][0]);
		mfma_settle(acc[mb][1]);
	}
#pragma unroll
	for (uint32_t mb = 0; mb < NMB; ++mb) {
		const bool valid = m0 + 16 * mb < a.M;
		const uint32_t m = m0 + (valid ? 16 * mb : 0u) + 4 * g;
#pragma unroll
		for (uint32_t sb = 0; sb < 2; ++sb) {
			const size_t sample = s0 + 32 * w + 16 * sb + lr;
			f4 o;
			if constexpr (EPI == G32_EPI_FORWARD || EPI == G32_EPI_FORWARD_TRIMMED) {
				o = act32_forward4<GENERAL>(a.act, acc[mb][sb]);
				if constexpr (EPI == G32_EPI_FORWARD) {
					if (valid && a.P) *(f4*)(a.P + sample * a.ldy + m) = acc[mb][sb];  // the saved pre-activation (SiLU / Sine, training)
				}
			} else if constexpr (EPI == G32_EPI_BACKWARD) {
				const f4 fv = *(const f4*)(a.F + sample * a.ldf + m);
				o = act32_backward4<GENERAL>(a.act, acc[mb][sb], fv);
			} else {
				o = acc[mb][sb];
			}
			if (valid) {
				if constexpr (EPI == G32_EPI_FORWARD_TRIMMED) {
					g32_store_trimmed(a, sample, m, o);
				} else if constexpr (Y_FM) {
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) a.Y[(size_t)(m + r) * a.n + sample] = o[r];
				} else {
					*(f4*)(a.Y + sample * a.ldy + m) = o;
				}
			}
		}
	}
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t G32_WG_TILE = 64;                  // out x in tile of a workgroup
constexpr uint32_t G32_WG_BS = 32;                    // samples per LDS stage
constexpr uint32_t G32_WG_LDT = G32_WG_TILE + 16;     // row stride of the sample-major stages [sample][feature]
constexpr uint32_t G32_WG_LDF = G32_WG_BS + 4;        // row stride of the feature-major stage [feature][sample] (the network input)
constexpr uint32_t G32_WG_STAGE = 2 * G32_WG_BS * G32_WG_LDT;

struct Gen32WgradArgs {
	uint32_t n, WO, WI;
	const float* d;       // sample-major [n][ldd], WO columns used
	uint32_t ldd;
	const float* a;       // sample-major [n][lda], or feature-major [WI][n] (A_FM)
	uint32_t lda;
	float* partials;
	size_t slab_stride, matrix_offset;
	uint32_t n_slices;
};

template <bool A_FM>
__global__ void __launch_bounds__(G32_THREADS) k_mlp_f32_wgrad(const Gen32WgradArgs p) {
	constexpr uint32_t T = G32_WG_TILE, BS = G32_WG_BS, LDT = G32_WG_LDT, LDF = G32_WG_LDF, CK = T / 4, CS = BS / 4;
	constexpr uint32_t PER = BS * CK / G32_THREADS;  // 16-byte chunks per thread, operand and stage
	static_assert(T * CS == BS * CK && T * LDF <= BS * LDT, "the feature-major stage has the sample-major one's chunks and room");
	TCNN_DYN_LDS(lds_raw);
	float* lds = (float*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t wo = w >> 1, wi = w & 1u;  // this wave's 32 x 32 quarter of the tile
	const uint32_t n_ti = div_round_up(p.WI, T), n_tiles = div_round_up(p.WO, T) * n_ti;
	const uint32_t tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;
	const uint32_t o0 = (tile / n_ti) * T, i0 = (tile % n_ti) * T;
	const uint32_t n_stages = p.n / BS;
	const uint32_t t_begin = (uint32_t)((uint64_t)slice * n_stages / p.n_slices), t_end = (uint32_t)((uint64_t)(slice + 1) * n_stages / p.n_slices);
	const f4 zero = zero4();

	f4 dreg[PER], areg[PER];
	auto load = [&](uint32_t t) {
		const size_t s = (size_t)t * BS;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS;
			{
				const uint32_t row = c / CK, cc = c % CK;
				const bool valid = o0 + 4 * cc < p.WO;
				const f4 v = *(const f4*)(p.d + (s + row) * p.ldd + (valid ? o0 + 4 * cc : 0u));
				dreg[q] = valid ? v : zero;
			}
			if constexpr (A_FM) {  // row = feature, cc = block of 4 samples
				const uint32_t row = c / CS, cc = c % CS;
				const bool valid = i0 + row < p.WI;
				const f4 v = *(const f4*)(p.a + (size_t)(valid ? i0 + row : 0u) * p.n + s + 4 * cc);
				areg[q] = valid ? v : zero;
			} else {
				const uint32_t row = c / CK, cc = c % CK;
				const bool valid = i0 + 4 * cc < p.WI;
				const f4 v = *(const f4*)(p.a + (s + row) * p.lda + (valid ? i0 + 4 * cc : 0u));
				areg[q] = valid ? v : zero;
			}
		}
	};
	auto store = [&](float* stage) {
		float* dT = stage;
		float* aT = stage + BS * LDT;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * G32_THREADS;
			*(f4*)(dT + (c / CK) * LDT + 4 * (c % CK)) = dreg[q];
			if constexpr (A_FM) {
				*(f4*)(aT + (c / CS) * LDF + 4 * (c % CS)) = areg[q];
			} else {
				*(f4*)(aT + (c / CK) * LDT + 4 * (c % CK)) = areg[q];
			}
		}
	};

	f4 acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
	if (t_begin < t_end) {
		load(t_begin);
		store(lds);
	}
	__syncthreads();
	for (uint32_t t = t_begin; t < t_end; ++t) {
		const float* dT = lds + ((t - t_begin) & 1u) * G32_WG_STAGE;
		const float* aT = dT + BS * LDT;
		const bool more = t + 1 < t_end;
		if (more) load(t + 1);
#pragma unroll
		for (uint32_t q = 0; q < BS / 4; ++q) {  // samples 4 q + g of the stage are this MFMA's k
			float av[2], bv[2];
#pragma unroll
			for (uint32_t b = 0; b < 2; ++b) {
				av[b] = dT[(4 * q + g) * LDT + 32 * wo + 16 * b + lr];
				if constexpr (A_FM) {
					bv[b] = aT[(32 * wi + 16 * b + lr) * LDF + 4 * q + g];
				} else {
					bv[b] = aT[(4 * q + g) * LDT + 32 * wi + 16 * b + lr];
				}
			}
#pragma unroll
			for (uint32_t oi = 0; oi < 2; ++oi)
#pragma unroll
				for (uint32_t ii = 0; ii < 2; ++ii) acc[oi][ii] = mfma_16x16x4_f32(av[oi], bv[ii], acc[oi][ii]);
		}
		if (more) store(lds + ((t + 1 - t_begin) & 1u) * G32_WG_STAGE);
		__syncthreads();
	}

	// this slice's slab, parameter order; accumulator element r <-> (out = 4 g + r, in = lr) of its 16 x 16 block.  Every block inside the
	// matrix is written by every slice (zeros from a slice without samples): k_mlp_f32_finalize reads all of them.
	float* P = p.partials + (size_t)slice * p.slab_stride + p.matrix_offset;
#pragma unroll
	for (uint32_t oi = 0; oi < 2; ++oi) {
#pragma unroll
		for (uint32_t ii = 0; ii < 2; ++ii) {
			const uint32_t ob = o0 + 32 * wo + 16 * oi, ib = i0 + 32 * wi + 16 * ii;
			f4 v = acc[oi][ii];
			mfma_settle(v);  // read on the far side of the branch below
			if (ob < p.WO && ib < p.WI) {
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) P[(size_t)(ob + 4 * g + r) * p.WI + ib + lr] = v[r];
			}
		}
	}
}

// ---- element-wise helpers: one thread per value (n_params and n * padded_out are multiples of 256) -----------------------------------
__global__ void __launch_bounds__(G32_THREADS) k_mlp_f32_finalize(uint32_t n_params, uint32_t n_partials, const float* partials, float* grads, uint32_t accumulate) {
	const uint32_t i = blockIdx.x * G32_THREADS + threadIdx.x;
	if (i >= n_params) return;
	float s = partials[i];
	for (uint32_t b = 1; b < n_partials; ++b) s += partials[(size_t)b * n_params + i];
	grads[i] = accumulate ? grads[i] + s : s;
}
__global__ void __launch_bounds__(G32_THREADS) k_mlp_f32_transpose(const MlpMeta m, const float* params, float* params_t) {
	const uint32_t i = blockIdx.x * G32_THREADS + threadIdx.x;
	if (i < m.n_params()) params_t[mlp_transposed_index(m, i)] = params[i];
}
__global__ void __launch_bounds__(G32_THREADS) k_mlp_f32_output_activation_backward(uint32_t n_fragments, uint32_t act, const float* output, const float* dL_doutput, float* dL_dpreact) {
	const uint32_t i = blockIdx.x * G32_THREADS + threadIdx.x;
	if (i >= n_fragments) return;
	const f4 y = *(const f4*)(output + 4 * (size_t)i), v = *(const f4*)(dL_doutput + 4 * (size_t)i);
	f4 o = act32_backward4_general(act, v, y);
	*(f4*)(dL_dpreact + 4 * (size_t)i) = o;
}

// =====================================================================================================================================
// host launchers
// =====================================================================================================================================
// blocks of 16 m per workgroup tile: the count in {4, 3, 2} that pads M least (ties: the larger tile)
static uint32_t g32_pick_nmb(uint32_t M) {
	const uint32_t q = M / 16u;
	if (q <= 1u) return 1u;
	uint32_t best = G32_MAX_MB, best_padded = next_multiple(q, G32_MAX_MB);
	for (uint32_t nmb = G32_MAX_MB - 1; nmb >= 2u; --nmb) {
		if (next_multiple(q, nmb) < best_padded) {
			best = nmb;
			best_padded = next_multiple(q, nmb);
		}
	}
	return best;
}

template <uint32_t EPI, bool X_FM, bool Y_FM>
static void g32_launch_layer(hipStream_t stream, const Gen32LayerArgs& a) {
	const uint32_t nmb = g32_pick_nmb(a.M);
	const dim3 grid(div_round_up(a.M, 16u * nmb) * (a.n / G32_BN)), block(G32_THREADS);
	const uint32_t lds_bytes = 2u * (16u * nmb + G32_BN) * G32_LDK * (uint32_t)sizeof(float);  // <= 54 KiB
	const bool general = EPI != G32_EPI_NONE && !act_is_simple(a.act);
#define TCNN_G32_LAUNCH(NMB_)                                                                                         \
	if (general) {                                                                                                    \
		TCNN_LAUNCH((k_mlp_f32_layer<NMB_, EPI, X_FM, Y_FM, EPI != G32_EPI_NONE>), grid, block, lds_bytes, stream, a); \
	} else {                                                                                                          \
		TCNN_LAUNCH((k_mlp_f32_layer<NMB_, EPI, X_FM, Y_FM, false>), grid, block, lds_bytes, stream, a);              \
	}
	switch (nmb) {
		case 1: TCNN_G32_LAUNCH(1) break;
		case 2: TCNN_G32_LAUNCH(2) break;
		case 3: TCNN_G32_LAUNCH(3) break;
		default: TCNN_G32_LAUNCH(4) break;
	}
#undef TCNN_G32_LAUNCH
}

// floats per store of g32_store_trimmed: rows start stride_i floats apart and a fragment at a multiple of 4 columns, so with unit column
// stride a 16-byte (8-byte) store is aligned everywhere iff the base is and stride_i is a multiple of 4 (2)
static uint32_t g32_trimmed_vec(const MlpF32Output& f) {
	if (f.stride_j != 1u) return 1u;
	const uintptr_t base = (uintptr_t)f.out;
	if (base % 16u == 0u && f.stride_i % 4u == 0u) return 4u;
	if (base % 8u == 0u && f.stride_i % 2u == 0u) return 2u;
	return 1u;
}

static void g32_check_shape(const MlpMeta& m, uint32_t n) {
	if (m.width % 16u != 0u || m.width == 0u || m.width > MLP_GENERAL_MAX_WIDTH || m.in_width % 16u != 0u || m.in_width == 0u || m.in_width > MLP_GENERAL_MAX_IN_WIDTH ||
	    m.padded_out % 16u != 0u || m.padded_out == 0u || m.padded_out > MLP_GENERAL_MAX_OUT_WIDTH) {
		throw std::runtime_error("mlp_f32: widths must be multiples of 16 within the layer-by-layer network's limits");
	}
	if (n % G32_BN != 0u) throw std::runtime_error("mlp_f32: the batch size must be a multiple of 128");
}

void mlp_f32_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* input, float* hidden, float* output, const MlpF32Output& trimmed) {
	g32_check_shape(m, n);
	const uint32_t W = m.width, HM = m.n_hidden_matmuls;
	if (trimmed.out && (hidden || output)) throw std::runtime_error("mlp_f32_forward: the trimmed output is for inference, in place of the padded one");
	if (trimmed.out && (trimmed.dims == 0 || trimmed.dims > m.padded_out)) throw std::runtime_error("mlp_f32_forward: the trimmed output has at most padded_out columns");
	// inference keeps two ping-pong activation matrices [n][W] instead of the saved stack: stream-ordered scratch of this call
	const size_t layer_elems = (size_t)n * W;
	float* ping = nullptr;
#if defined(TCNN_HOST_EMU)
	std::vector<float> ping_host;
	if (!hidden) {
		ping_host.resize(2 * layer_elems);
		ping = ping_host.data();
	}
#else
	Scratch ping_scratch;
	if (!hidden) {
		ping_scratch = Scratch(stream, 2 * layer_elems * sizeof(float));
		ping = ping_scratch.as<float>();
	}
#endif
	// SiLU / Sine: the saved stack has a second block, the pre-activations; inference saves neither
	float* pre_block = act_needs_preactivation(m.activation) && hidden ? hidden + (HM + 1) * layer_elems : nullptr;
	const float* Wl = params;
	const float* x = input;
	uint32_t K = m.in_width;
	for (uint32_t layer = 0; layer <= HM; ++layer) {
		float* y = hidden ? hidden + layer * layer_elems : ping + (layer & 1u) * layer_elems;
		const Gen32LayerArgs a = {n, W, K, Wl, x, K, y, W, nullptr, 0u, m.activation, pre_block ? pre_block + layer * layer_elems : nullptr, nullptr, 0u, 0u, 0u, 0u};
		if (layer == 0) {
			g32_launch_layer<G32_EPI_FORWARD, true, false>(stream, a);  // the network input is feature-major
		} else {
			g32_launch_layer<G32_EPI_FORWARD, false, false>(stream, a);
		}
		Wl += (size_t)W * K;
		x = y;
		K = W;
	}
	Gen32LayerArgs a = {n, m.padded_out, W, Wl, x, W, output, m.padded_out, nullptr, 0u, m.output_activation, nullptr, nullptr, 0u, 0u, 0u, 0u};
	if (trimmed.out) {
		a.Yt = trimmed.out;
		a.t_dims = trimmed.dims;
		a.t_stride_i = trimmed.stride_i;
		a.t_stride_j = trimmed.stride_j;
		a.t_vec = g32_trimmed_vec(trimmed);
		g32_launch_layer<G32_EPI_FORWARD_TRIMMED, false, false>(stream, a);
	} else {
		g32_launch_layer<G32_EPI_FORWARD, false, false>(stream, a);
	}
}

void mlp_f32_transpose_weights(hipStream_t stream, const MlpMeta& m, const float* params, float* params_t) {
	TCNN_LAUNCH(k_mlp_f32_transpose, dim3(div_round_up(m.n_params(), G32_THREADS)), dim3(G32_THREADS), 0, stream, m, params, params_t);
}

void mlp_f32_output_activation_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* output, const float* dL_doutput, float* dL_dpreact) {
	const uint64_t fragments = (uint64_t)n * m.padded_out / 4u;
	if (fragments > 0xFFFFFFFFull) throw std::runtime_error("mlp_f32_output_activation_backward: the batch is too large; split it");
	if (fragments == 0) return;
	TCNN_LAUNCH(k_mlp_f32_output_activation_backward, dim3(div_round_up((uint32_t)fragments, G32_THREADS)), dim3(G32_THREADS), 0, stream, (uint32_t)fragments,
	            m.output_activation, output, dL_doutput, dL_dpreact);
}

// The fp32 slabs of all slices may take this much scratch (mlp_general.hip: the same budget, target and bound).
constexpr size_t G32_SLAB_BUDGET_BYTES = (size_t)128 << 20;
constexpr uint32_t G32_WG_TARGET_BLOCKS = 1024;
constexpr uint32_t G32_WG_MAX_SLICES = 32;

static uint32_t g32_wgrad_tiles(uint32_t WO, uint32_t WI) { return div_round_up(WO, G32_WG_TILE) * div_round_up(WI, G32_WG_TILE); }

uint32_t mlp_f32_n_partials(const MlpMeta& m, uint32_t n) {
	const uint32_t tiles = std::max(g32_wgrad_tiles(m.width, m.width), g32_wgrad_tiles(m.width, m.in_width));
	const size_t by_budget = G32_SLAB_BUDGET_BYTES / ((size_t)m.n_params() * sizeof(float));
	uint32_t wanted = std::min(div_round_up(G32_WG_TARGET_BLOCKS, tiles), G32_WG_MAX_SLICES);
	wanted = std::min(wanted, std::max(n / G32_WG_BS, 1u));
	wanted = (uint32_t)std::min<size_t>(wanted, std::max<size_t>(by_budget, 1));
	uint32_t slices = 1;
	while (slices * 2u <= wanted) slices *= 2u;
	return slices;
}

size_t mlp_f32_backward_workspace_bytes(const MlpMeta& m, uint32_t n) { return (size_t)(m.n_hidden_matmuls + 1) * n * m.width * sizeof(float); }

void mlp_f32_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* input, const float* hidden, const float* dL_doutput,
                      float* dL_dinput, float* partials, void* workspace) {
	g32_check_shape(m, n);
	if (!workspace) throw std::runtime_error("mlp_f32_backward: a workspace is required (mlp_f32_backward_workspace_bytes)");
	if (!hidden) throw std::runtime_error("mlp_f32_backward: the saved activations of the forward pass are required");
	const uint32_t W = m.width, IN = m.in_width, HM = m.n_hidden_matmuls, OUTP = m.padded_out;
	const size_t layer_elems = (size_t)n * W;
	float* dact = (float*)workspace;  // [n_hidden][n][W]
	const float* wt_in = params_t;                              // [IN][W]
	const float* wt_hid = wt_in + (size_t)IN * W;               // HM x [W][W]  (row = input neuron of the matrix)
	const float* wt_out = wt_hid + (size_t)HM * W * W;          // [W][OUTP]

	// dA_last = (dY W_out) * act'(A_last), then down the hidden matrices.  The derivative is taken at the saved post-activations, or -- SiLU /
	// Sine -- at the pre-activations in the stack's second block; the weight-gradient products below read the first block either way.
	const float* at = act_needs_preactivation(m.activation) ? hidden + (HM + 1) * layer_elems : hidden;
	auto derivative_layer = [&](uint32_t K, const float* wt, const float* x, uint32_t j) {
		const Gen32LayerArgs a = {n, W, K, wt, x, K, dact + j * layer_elems, W, at + j * layer_elems, W, m.activation, nullptr, nullptr, 0u, 0u, 0u, 0u};
		g32_launch_layer<G32_EPI_BACKWARD, false, false>(stream, a);
	};
	derivative_layer(OUTP, wt_out, dL_doutput, HM);
	for (uint32_t j = HM; j-- > 0;) derivative_layer(W, wt_hid + (size_t)j * W * W, dact + (j + 1) * layer_elems, j);
	if (dL_dinput) {  // no activation on the network input; feature-major like the input
		const Gen32LayerArgs a = {n, IN, W, wt_in, dact, W, dL_dinput, 0u, nullptr, 0u, (uint32_t)Activation::None, nullptr, nullptr, 0u, 0u, 0u, 0u};
		g32_launch_layer<G32_EPI_NONE, false, true>(stream, a);
	}
	if (!partials) return;

	const uint32_t n_slices = mlp_f32_n_partials(m, n);
	const size_t slab = m.n_params(), off_hid = (size_t)W * IN, off_out = off_hid + (size_t)HM * W * W;
	const uint32_t lds_bytes = 2u * G32_WG_STAGE * (uint32_t)sizeof(float);  // 40 KiB
	auto product = [&](uint32_t WO, uint32_t WI, const float* d, uint32_t ldd, const float* a, uint32_t lda, bool a_fm, size_t offset) {
		const Gen32WgradArgs p = {n, WO, WI, d, ldd, a, lda, partials, slab, offset, n_slices};
		const dim3 grid(g32_wgrad_tiles(WO, WI) * n_slices), block(G32_THREADS);
		if (a_fm) {
			TCNN_LAUNCH((k_mlp_f32_wgrad<true>), grid, block, lds_bytes, stream, p);
		} else {
			TCNN_LAUNCH((k_mlp_f32_wgrad<false>), grid, block, lds_bytes, stream, p);
		}
	};
	product(OUTP, W, dL_doutput, OUTP, hidden + HM * layer_elems, W, false, off_out);
	for (uint32_t j = 0; j < HM; ++j) product(W, W, dact + (j + 1) * layer_elems, W, hidden + j * layer_elems, W, false, off_hid + (size_t)j * W * W);
	product(W, IN, dact, W, input, 0u, true, 0);  // the input matrix: a = the feature-major network input
}

void mlp_f32_finalize_gradients(hipStream_t stream, const MlpMeta& m, uint32_t n_partials, const float* partials, float* grads, bool accumulate) {
	if (n_partials == 0) throw std::runtime_error("mlp_f32_finalize_gradients: no slabs");
	TCNN_LAUNCH(k_mlp_f32_finalize, dim3(div_round_up(m.n_params(), G32_THREADS)), dim3(G32_THREADS), 0, stream, m.n_params(), n_partials, partials, grads,
	            accumulate ? 1u : 0u);
}

}  // namespace tcnn_hip

// mlp_general_impl.h -- the layer-by-layer network, ONE source for the 16-bit type (half_t) and for float, instantiated by two units
// (mlp_general.hip: half_t; mlp_general_fp32.hip: float -- two code objects, as the kernels were laid out and measured):
//   * 16-bit: what the fused kernels are not built for (mlp_kernels.h mlp_layer_by_layer): hidden widths that are a multiple of 16 up to
//     MLP_GENERAL_MAX_WIDTH other than 16 / 32 / 64 / 128, and -- at every width -- the hidden activations whose derivative needs the
//     pre-activation (SiLU, Sine) and more than MLP_MAX_OUT_WIDTH padded outputs (up to MLP_GENERAL_MAX_OUT_WIDTH: the output matrix is one
//     more M x K product, the weight-gradient tiles cover any row count).  v_mfma_f32_16x16x32_f16 / _bf16.
//   * fp32 (mlp_kernels.h mlp_f32_*): weights, activations and gradients are float, every product runs on v_mfma_f32_16x16x4_f32 and nothing
//     is rounded between the accumulator and the store.
// Stands where the reference's CutlassMLP stands (cutlass_mlp.cu:110-330: one GEMM with an activation epilogue per layer, one GEMM per layer
// for dL/d(pre-activation), one split-K GEMM per weight matrix) -- its BEHAVIOUR, not its tiling.  Same parameter layout, transposed scratch
// and boundary layouts as the fused kernels (mlp_kernels.h), so everything above the launchers is shared.  What differs between the two
// precisions is in Gen<T>, which each unit specialises; the kernels, their argument blocks and the host code are templates over it.
//
// Two kernels:
//   * k_mlp_general_layer:  Y[sample][m] = epilogue(sum_k Wm[m][k] X[sample][k]) for one matrix Wm [M][K] row-major.  Forward: Wm = a
//     layer's weights, epilogue = activation.  Backward: Wm = the TRANSPOSED weights (params_t), X = dL/d(pre-activation) of the layer
//     above, epilogue = the activation's derivative on the saved post-activation values.  SiLU / Sine, 16-bit (the _PRE epilogues): forward
//     rounds the accumulator to 16 bits, stores it into the stack's second block (training) and applies the activation to the rounded value;
//     backward multiplies the rounded accumulator by the rounded derivative at that saved pre-activation.  SiLU / Sine, fp32: the general
//     epilogues -- forward stores the accumulator as the pre-activation as well, backward takes the derivative at it.
//     Both operands have k contiguous, so the weights are the MFMA A operand and the activations the B operand straight out of [row][k] LDS
//     tiles: a lane reads one 16-byte chunk per operand block (8 k of the 16x16x32 shape; 4 k of its row, element j of which goes to the j-th
//     of four 16x16x4 MFMAs -- which k a lane's element stands for is free as long as A and B agree), and the accumulator fragment (4
//     consecutive m for one sample) is ONE store into the sample-major result.  The output layer of an inference into the caller's fp32
//     matrix (GEN_EPI_FORWARD_TRIMMED, MlpF32Output) stores the columns below the unpadded width with the caller's strides; 16-bit: rounded
//     like the 16-bit store and widened -- the bits of the padded 16-bit matrix put through trim_and_cast, without the matrix.
//     Workgroup: 4 waves, tile = (16 * NMB m) x (128 samples); wave w owns samples 32w .. 32w+31 and all NMB blocks of m (2 B reads + NMB
//     A reads per 2 * NMB (fp32: 8 * NMB) MFMAs; 2 * NMB independent accumulators cover the fp32 shape's 40-cycle dependent latency).  K runs
//     in steps of 128 bytes a row through two LDS stages: the global loads of step s + 1 are issued into registers before the MFMAs of step
//     s and written to the other stage after them -- one barrier per step.  Rows of 144 bytes: the 16 rows of a 16-byte fragment read start
//     36 banks apart, i.e. on 16 different 4-bank slots -- conflict-free.  LDS: 2 * (64 + 128) * 144 B = 54 KiB at NMB = 4 (two workgroups
//     per CU), whatever the network's width.
//   * k_mlp_general_wgrad:  dW[o][i] = sum_s d[s][o] a[s][i] for one 64 x 64 tile of one matrix over one slice of the batch.  Both operands
//     arrive sample-major (k = the sample is the STRIDED index) and are staged as they lie, with 16-byte copies.  16-bit: turned into
//     "samples in k" fragments by the hardware transpose read (lds_read_tr4); group g of a wave reads rows 4g .. 4g+3 and 16+4g .. 16+4g+3 of
//     a 32-sample step, so the 8 rows a half wave touches per read are consecutive, and with rows of 64 + 16 halves (40 dwords) they start 8
//     banks apart -- conflict-free.  fp32: one float per lane and operand, so the fragment is a plain 4-byte read of row 4 q + g, column lr;
//     rows of 64 + 16 floats put the four rows of a read 16 banks apart -- conflict-free.  The feature-major network input is staged
//     [feature][sample] in rows of 144 bytes.  Two stages of 20 KiB.
//     The batch is cut into a fixed number of slices (gen_n_partials); slice s writes its tiles into fp32 slab s in parameter order, and
//     mlp_finalize_gradients / k_mlp_f32_finalize sum the slabs in fixed order: deterministic, no floating-point atomics.
#pragma once
#include "mlp_kernels.h"

#if !defined(TCNN_HOST_EMU)
#include "scratch_cache.h"
#endif

#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace tcnn_hip {

constexpr uint32_t GEN_THREADS = 256;
constexpr uint32_t GEN_BN = 128;           // samples per workgroup tile of k_mlp_general_layer
constexpr uint32_t GEN_MAX_MB = 4;         // blocks of 16 m per workgroup tile, at most
constexpr uint32_t GEN_WG_TILE = 64;       // out x in tile of a workgroup of k_mlp_general_wgrad

// ---- what differs between the two precisions ----------------------------------------------------------------------------------------
template <typename T>
struct GenTile {
	static constexpr uint32_t VE = 16 / sizeof(T);                 // elements of a 16-byte chunk
	static constexpr uint32_t BK = 8 * VE;                         // k per LDS stage of the layer kernel: 64 halves / 32 floats
	static constexpr uint32_t LDK = BK + VE;                       // row stride of its [row][k] stages: 144 bytes
	static constexpr uint32_t WG_BS = 8 * VE;                      // samples per LDS stage of the weight-gradient kernel
	static constexpr uint32_t WG_LDT = GEN_WG_TILE + 16;           // row stride of its sample-major stages [sample][feature]
	static constexpr uint32_t WG_LDF = WG_BS + VE;                 // row stride of its feature-major stage [feature][sample] (the network input)
	static constexpr uint32_t WG_STAGE = 2 * WG_BS * WG_LDT;
};
template <typename T>
struct Gen;

// _PRE (16-bit only): the epilogues of the activations that keep their pre-activation (SiLU / Sine, activation_device.h act_forward4_pre /
// act_backward4_pre).  _TRIMMED: GEN_EPI_FORWARD whose result goes to the caller's fp32 matrix (Yt ...) instead of Y
// _DERIVATIVE_RAW / _CURVATURE (fp32 only): the epilogues of the second-order pass (gen_backward_backward below).  _DERIVATIVE_RAW is
// GEN_EPI_BACKWARD that also keeps the raw accumulator (through P); _CURVATURE adds the term with the activation's second derivative.
enum : uint32_t {
	GEN_EPI_NONE = 0, GEN_EPI_FORWARD = 1, GEN_EPI_BACKWARD = 2, GEN_EPI_FORWARD_PRE = 3, GEN_EPI_BACKWARD_PRE = 4, GEN_EPI_FORWARD_TRIMMED = 5,
	GEN_EPI_DERIVATIVE_RAW = 6, GEN_EPI_CURVATURE = 7
};

template <typename T>
struct GenLayerArgs {
	uint32_t n, M, K;
	const T* Wm;          // [M][K] row-major
	const T* X;           // sample-major [n][ldx], or feature-major [K][n] (X_FM)
	uint32_t ldx;
	T* Y;                 // sample-major [n][ldy], or feature-major [M][n] (Y_FM)
	uint32_t ldy;
	const T* F;           // GEN_EPI_BACKWARD, _DERIVATIVE_RAW, _CURVATURE: the values the derivative is taken at, sample-major [n][ldf]:
	uint32_t ldf;         // post-activations (fp32 SiLU / Sine: pre-activations).  GEN_EPI_BACKWARD_PRE: the PRE-activation values, same layout
	uint32_t act;
	T* P;                 // GEN_EPI_FORWARD_PRE, fp32 GEN_EPI_FORWARD: where the pre-activations go, sample-major [n][ldy]; null: not saved.
	                      // GEN_EPI_DERIVATIVE_RAW: where the raw accumulator goes, same layout; null: not kept
	// GEN_EPI_FORWARD_TRIMMED: element (sample i, m) with m < t_dims at Yt[i * t_stride_i + m * t_stride_j].  t_vec: floats per store the host
	// proved aligned for EVERY (sample, m = multiple of 4) -- 4 or 2 only with t_stride_j == 1 (gen_trimmed_vec) -- else 1
	float* Yt;
	uint32_t t_dims, t_stride_i, t_stride_j, t_vec;
	// GEN_EPI_CURVATURE: Y = acc * act'(F) + E * Tn * act''(F), the two factors sample-major [n][ldy] like Y.  Y may BE E (each fragment is
	// read and written by the one lane that holds it, the reads first)
	const T* E;
	const T* Tn;
};

// the 4 values of one accumulator fragment (m .. m + 3 of one sample) into the caller's fp32 matrix: one 16-byte store where the host
// proved that alignment and all 4 columns exist; else 8-byte stores per existing pair where it proved that, a lone last column on its own;
// else column by column.  Nothing at or past t_dims is written.
template <typename T>
TCNN_DEVICE void gen_store_trimmed(const GenLayerArgs<T>& a, size_t sample, uint32_t m, f4 v) {
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

template <typename T, uint32_t NMB, uint32_t EPI, bool X_FM, bool Y_FM, bool GENERAL>
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_general_layer(const GenLayerArgs<T> a) {
	typedef Gen<T> G;
	typedef typename G::vec vec;
	typedef typename G::frag frag;
	static_assert(G::PRE_EPILOGUES || (EPI != GEN_EPI_FORWARD_PRE && EPI != GEN_EPI_BACKWARD_PRE), "the fp32 network has no _PRE instances");
	static_assert(!G::PRE_EPILOGUES || (EPI != GEN_EPI_DERIVATIVE_RAW && EPI != GEN_EPI_CURVATURE), "the second-order pass is the fp32 network's");
	constexpr uint32_t VE = G::VE, BK = G::BK, LDK = G::LDK, KR = 4 * VE;  // KR: k per operand read of a wave (4 lane groups x one chunk)
	constexpr uint32_t BM = 16 * NMB, CK = BK / VE;                        // CK: 16-byte chunks per row of a stage
	constexpr uint32_t W_CHUNKS = BM * CK, X_CHUNKS = GEN_BN * CK;
	constexpr uint32_t W_PER = (W_CHUNKS + GEN_THREADS - 1) / GEN_THREADS, X_PER = X_CHUNKS / GEN_THREADS;
	constexpr uint32_t STAGE = (BM + GEN_BN) * LDK;
	TCNN_DYN_LDS(lds_raw);
	T* lds = (T*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t n_mt = div_round_up(a.M, BM);
	const uint32_t m0 = (blockIdx.x % n_mt) * BM;           // m tiles fastest: neighbouring workgroups share their sample tile in L2
	const size_t s0 = (size_t)(blockIdx.x / n_mt) * GEN_BN;
	const uint32_t n_steps = div_round_up(a.K, BK);
	const vec zero = G::zero();

	// one K step of both operands, global -> registers.  Chunks past M or K read a valid address and are replaced by zeros (K is a
	// multiple of 16, a chunk is 8 or 4: wholly inside or outside).  Written as a select; what hipcc makes of it follows Gen<T>::zero():
	// selects behind unconditional loads in the 16-bit kernels, branches around the loads in the fp32 ones.
	vec wreg[W_PER], xreg[X_PER];
	auto load = [&](uint32_t k0) {
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, kc = c % CK;
			const bool valid = c < W_CHUNKS && m0 + row < a.M && k0 + VE * kc < a.K;
			const vec v = *(const vec*)(a.Wm + (valid ? (size_t)(m0 + row) * a.K + k0 + VE * kc : (size_t)0));
			wreg[q] = valid ? v : zero;
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			if constexpr (X_FM) {  // consecutive lanes = consecutive features: the transposing element stores below fall into one row
				const uint32_t k = c % BK, sc = c / BK;
				const bool valid = k0 + k < a.K;
				const vec v = *(const vec*)(a.X + (size_t)(valid ? k0 + k : 0u) * a.n + s0 + VE * sc);
				xreg[q] = valid ? v : zero;
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				const bool valid = k0 + VE * kc < a.K;
				const vec v = *(const vec*)(a.X + (s0 + row) * a.ldx + (valid ? k0 + VE * kc : 0u));
				xreg[q] = valid ? v : zero;
			}
		}
	};
	auto store = [&](T* stage) {
		T* Wt = stage;
		T* Xt = stage + BM * LDK;
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, kc = c % CK;
			if (c < W_CHUNKS) *(vec*)(Wt + row * LDK + VE * kc) = wreg[q];
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			if constexpr (X_FM) {
				const uint32_t k = c % BK, sc = c / BK;
#pragma unroll
				for (uint32_t j = 0; j < VE; ++j) Xt[(VE * sc + j) * LDK + k] = xreg[q][j];
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				*(vec*)(Xt + row * LDK + VE * kc) = xreg[q];
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
		const T* Wt = lds + (ks & 1u) * STAGE;
		const T* Xt = Wt + BM * LDK;
		const bool more = ks + 1 < n_steps;
		if (more) load((ks + 1) * BK);  // in flight while the MFMAs below run
#pragma unroll
		for (uint32_t kk = 0; kk < BK / KR; ++kk) {
			vec bv[2];
#pragma unroll
			for (uint32_t sb = 0; sb < 2; ++sb) bv[sb] = *(const vec*)(Xt + (32 * w + 16 * sb + lr) * LDK + KR * kk + VE * g);
#pragma unroll
			for (uint32_t mb = 0; mb < NMB; ++mb) {
				const vec av = *(const vec*)(Wt + (16 * mb + lr) * LDK + KR * kk + VE * g);
#pragma unroll
				for (uint32_t j = 0; j < KR / G::MFMA_K; ++j)  // one 16x16x32 on the chunk, or four 16x16x4 on its elements
#pragma unroll
					for (uint32_t sb = 0; sb < 2; ++sb) acc[mb][sb] = G::mfma(G::part(av, j), G::part(bv[sb], j), acc[mb][sb]);
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
			frag o;
			if constexpr (EPI == GEN_EPI_FORWARD || EPI == GEN_EPI_FORWARD_TRIMMED) {
				o = G::template forward<GENERAL>(a.act, acc[mb][sb]);
				if constexpr (EPI == GEN_EPI_FORWARD && !G::PRE_EPILOGUES) {
					if (valid && a.P) *(frag*)(a.P + sample * a.ldy + m) = G::narrow(acc[mb][sb]);  // the saved pre-activation (SiLU / Sine, training)
				}
			} else if constexpr (EPI == GEN_EPI_BACKWARD) {
				const frag fv = *(const frag*)(a.F + sample * a.ldf + m);
				o = G::template backward<GENERAL>(a.act, acc[mb][sb], fv);
			} else if constexpr (EPI == GEN_EPI_DERIVATIVE_RAW) {
				// the tangent pass (forward weights: t and u = t * act') and the first-order recomputation (transposed weights: e and d = e * act')
				const frag fv = *(const frag*)(a.F + sample * a.ldf + m);
				o = G::template backward<GENERAL>(a.act, acc[mb][sb], fv);
				if (valid && a.P) *(frag*)(a.P + sample * a.ldy + m) = G::narrow(acc[mb][sb]);
			} else if constexpr (EPI == GEN_EPI_CURVATURE) {
				// all three fragments in flight before anything is computed or stored; no element-wise pass over [n][W] beside the product
				const frag fv = *(const frag*)(a.F + sample * a.ldf + m);
				const frag ev = *(const frag*)(a.E + sample * a.ldy + m);
				const frag tv = *(const frag*)(a.Tn + sample * a.ldy + m);
				o = G::curvature(a.act, acc[mb][sb], ev, tv, fv);
			} else if constexpr (EPI == GEN_EPI_FORWARD_PRE) {
				// one launch where the reference runs a product and an element-wise pass: the rounded accumulator is the saved
				// pre-activation AND the activation's argument.  Both stores behind everything this iteration computes; it loads nothing.
				frag pre;
				o = act_forward4_pre(a.act, acc[mb][sb], pre);
				if (valid && a.P) *(frag*)(a.P + sample * a.ldy + m) = pre;
			} else if constexpr (EPI == GEN_EPI_BACKWARD_PRE) {
				const frag pre = *(const frag*)(a.F + sample * a.ldf + m);
				o = act_backward4_pre(a.act, acc[mb][sb], pre);
			} else {
				o = G::narrow(acc[mb][sb]);
			}
			if (valid) {
				if constexpr (EPI == GEN_EPI_FORWARD_TRIMMED) {
					gen_store_trimmed(a, sample, m, G::widen(o));
				} else if constexpr (Y_FM) {
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) a.Y[(size_t)(m + r) * a.n + sample] = o[r];
				} else {
					*(frag*)(a.Y + sample * a.ldy + m) = o;
				}
			}
		}
	}
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------
template <typename T>
struct GenWgradArgs {
	uint32_t n, WO, WI;
	const T* d;           // sample-major [n][ldd], WO columns used
	uint32_t ldd;
	const T* a;           // sample-major [n][lda], or feature-major [WI][n] (A_FM)
	uint32_t lda;
	float* partials;
	size_t slab_stride, matrix_offset;
	uint32_t n_slices;
};
// with a second operand pair in the layouts of the first: the tile is sum_s d[s][o] a[s][i] + sum_s d2[s][o] a2[s][i].  An argument block of
// its own, so that the single-pair instances keep theirs (and their code) as they were
template <typename T>
struct GenWgradDualArgs : GenWgradArgs<T> {
	const T* d2;
	const T* a2;
};

// ARGS = GenWgradDualArgs (the second-order pass, mlp_f32_backward_backward): every slice runs its stages of the first pair, then the same
// stages of the second, into the same accumulators -- one launch and one slab entry per matrix element, the order of the terms fixed.
template <typename T, bool A_FM, typename ARGS = GenWgradArgs<T>>
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_general_wgrad(const ARGS p) {
	constexpr bool DUAL = !std::is_same<ARGS, GenWgradArgs<T>>::value;
	typedef Gen<T> G;
	typedef typename G::vec vec;
	constexpr uint32_t TILE = GEN_WG_TILE, VE = G::VE, BS = G::WG_BS, LDT = G::WG_LDT, LDF = G::WG_LDF, CK = TILE / VE, CS = BS / VE;
	constexpr uint32_t PER = BS * CK / GEN_THREADS;  // 16-byte chunks per thread, operand and stage
	static_assert(TILE * CS == BS * CK && TILE * LDF <= BS * LDT, "the feature-major stage has the sample-major one's chunks and room");
	TCNN_DYN_LDS(lds_raw);
	T* lds = (T*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t wo = w >> 1, wi = w & 1u;  // this wave's 32 x 32 quarter of the tile
	const uint32_t n_ti = div_round_up(p.WI, TILE), n_tiles = div_round_up(p.WO, TILE) * n_ti;
	const uint32_t tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;
	const uint32_t o0 = (tile / n_ti) * TILE, i0 = (tile % n_ti) * TILE;
	const uint32_t n_stages = p.n / BS;
	const uint32_t t_begin = (uint32_t)((uint64_t)slice * n_stages / p.n_slices), t_second = (uint32_t)((uint64_t)(slice + 1) * n_stages / p.n_slices);
	const uint32_t t_end = DUAL ? 2u * t_second - t_begin : t_second;  // DUAL: stage t >= t_second is stage t - (t_second - t_begin) of the second pair
	const vec zero = G::zero();

	vec dreg[PER], areg[PER];
	auto load = [&](uint32_t t) {
		const T* pd = p.d;
		const T* pa = p.a;
		if constexpr (DUAL) {
			if (t >= t_second) {  // (uniform)
				t -= t_second - t_begin;
				pd = p.d2;
				pa = p.a2;
			}
		}
		const size_t s = (size_t)t * BS;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			{
				const uint32_t row = c / CK, cc = c % CK;
				const bool valid = o0 + VE * cc < p.WO;
				const vec v = *(const vec*)(pd + (s + row) * p.ldd + (valid ? o0 + VE * cc : 0u));
				dreg[q] = valid ? v : zero;
			}
			if constexpr (A_FM) {  // row = feature, cc = chunk of samples
				const uint32_t row = c / CS, cc = c % CS;
				const bool valid = i0 + row < p.WI;
				const vec v = *(const vec*)(pa + (size_t)(valid ? i0 + row : 0u) * p.n + s + VE * cc);
				areg[q] = valid ? v : zero;
			} else {
				const uint32_t row = c / CK, cc = c % CK;
				const bool valid = i0 + VE * cc < p.WI;
				const vec v = *(const vec*)(pa + (s + row) * p.lda + (valid ? i0 + VE * cc : 0u));
				areg[q] = valid ? v : zero;
			}
		}
	};
	auto store = [&](T* stage) {
		T* dT = stage;
		T* aT = stage + BS * LDT;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			*(vec*)(dT + (c / CK) * LDT + VE * (c % CK)) = dreg[q];
			if constexpr (A_FM) {
				*(vec*)(aT + (c / CS) * LDF + VE * (c % CS)) = areg[q];
			} else {
				*(vec*)(aT + (c / CK) * LDT + VE * (c % CK)) = areg[q];
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
		const T* dT = lds + ((t - t_begin) & 1u) * G::WG_STAGE;
		const T* aT = dT + BS * LDT;
		const bool more = t + 1 < t_end;
		if (more) load(t + 1);
#pragma unroll
		for (uint32_t q = 0; q < BS / G::MFMA_K; ++q) {  // samples MFMA_K q .. of the stage are this MFMA's k
			typename G::operand av[2], bv[2];
#pragma unroll
			for (uint32_t b = 0; b < 2; ++b) {
				av[b] = G::wg_samples(dT, q, wo, b, LDT, lane, lr, g);
				if constexpr (A_FM) {
					bv[b] = G::wg_samples_fm(aT, q, wi, b, LDF, lane, lr, g);
				} else {
					bv[b] = G::wg_samples(aT, q, wi, b, LDT, lane, lr, g);
				}
			}
#pragma unroll
			for (uint32_t oi = 0; oi < 2; ++oi)
#pragma unroll
				for (uint32_t ii = 0; ii < 2; ++ii) acc[oi][ii] = G::mfma(av[oi], bv[ii], acc[oi][ii]);
		}
		if (more) store(lds + ((t + 1 - t_begin) & 1u) * G::WG_STAGE);
		__syncthreads();
	}

	// this slice's slab, parameter order; accumulator element r <-> (out = 4 g + r, in = lr) of its 16 x 16 block.  Every block inside the
	// matrix is written by every slice (zeros from a slice without samples): the finalize kernels read all of them.
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

// =====================================================================================================================================
// host launchers
// =====================================================================================================================================
// blocks of 16 m per workgroup tile: the count in {4, 3, 2} that pads M least (ties: the larger tile)
static uint32_t gen_pick_nmb(uint32_t M) {
	const uint32_t q = M / 16u;
	if (q <= 1u) return 1u;
	uint32_t best = GEN_MAX_MB, best_padded = next_multiple(q, GEN_MAX_MB);
	for (uint32_t nmb = GEN_MAX_MB - 1; nmb >= 2u; --nmb) {
		if (next_multiple(q, nmb) < best_padded) {
			best = nmb;
			best_padded = next_multiple(q, nmb);
		}
	}
	return best;
}

template <typename T, uint32_t EPI, bool X_FM, bool Y_FM>
static void gen_launch_layer(hipStream_t stream, const GenLayerArgs<T>& a) {
	const uint32_t nmb = gen_pick_nmb(a.M);
	const dim3 grid(div_round_up(a.M, 16u * nmb) * (a.n / GEN_BN)), block(GEN_THREADS);
	const uint32_t lds_bytes = 2u * (16u * nmb + GEN_BN) * Gen<T>::LDK * (uint32_t)sizeof(T);  // <= 54 KiB
	const bool general = EPI != GEN_EPI_NONE && !act_is_simple(a.act);
	// the _PRE and _CURVATURE epilogues have one instance per tile shape (GENERAL says nothing there: _CURVATURE is launched for the
	// activations with a second derivative only); the other instances are what they were
#define TCNN_GEN_LAUNCH(NMB_)                                                                                                   \
	if constexpr (EPI == GEN_EPI_FORWARD_PRE || EPI == GEN_EPI_BACKWARD_PRE || EPI == GEN_EPI_CURVATURE) {                      \
		TCNN_LAUNCH((k_mlp_general_layer<T, NMB_, EPI, X_FM, Y_FM, true>), grid, block, lds_bytes, stream, a);                  \
	} else if (general) {                                                                                                       \
		TCNN_LAUNCH((k_mlp_general_layer<T, NMB_, EPI, X_FM, Y_FM, EPI != GEN_EPI_NONE>), grid, block, lds_bytes, stream, a);   \
	} else {                                                                                                                    \
		TCNN_LAUNCH((k_mlp_general_layer<T, NMB_, EPI, X_FM, Y_FM, false>), grid, block, lds_bytes, stream, a);                 \
	}
	switch (nmb) {
		case 1: TCNN_GEN_LAUNCH(1) break;
		case 2: TCNN_GEN_LAUNCH(2) break;
		case 3: TCNN_GEN_LAUNCH(3) break;
		default: TCNN_GEN_LAUNCH(4) break;
	}
#undef TCNN_GEN_LAUNCH
}

// floats per store of gen_store_trimmed: rows start stride_i floats apart and a fragment at a multiple of 4 columns, so with unit column
// stride a 16-byte (8-byte) store is aligned everywhere iff the base is and stride_i is a multiple of 4 (2)
static uint32_t gen_trimmed_vec(const MlpF32Output& f) {
	if (f.stride_j != 1u) return 1u;
	const uintptr_t base = (uintptr_t)f.out;
	if (base % 16u == 0u && f.stride_i % 4u == 0u) return 4u;
	if (base % 8u == 0u && f.stride_i % 2u == 0u) return 2u;
	return 1u;
}

// the argument checks are each precision's own: mlp_general_forward / mlp_f32_forward below
template <typename T>
static void gen_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const T* params, const T* input, T* hidden, T* output, const MlpF32Output& trimmed) {
	const uint32_t W = m.width, HM = m.n_hidden_matmuls;
	// inference keeps two ping-pong activation matrices [n][W] instead of the saved stack: stream-ordered scratch of this call
	const size_t layer_elems = (size_t)n * W;
	T* ping = nullptr;
#if defined(TCNN_HOST_EMU)
	std::vector<T> ping_host;
	if (!hidden) {
		ping_host.resize(2 * layer_elems);
		ping = ping_host.data();
	}
#else
	Scratch ping_scratch;
	if (!hidden) {
		ping_scratch = Scratch(stream, 2 * layer_elems * sizeof(T));
		ping = ping_scratch.as<T>();
	}
#endif
	// SiLU / Sine: the saved stack has a second block, the pre-activations (mlp_saved_activation_bytes); inference saves neither
	const bool keeps_pre = act_needs_preactivation(m.activation);
	T* pre_block = keeps_pre && hidden ? hidden + (HM + 1) * layer_elems : nullptr;
	auto hidden_layer = [&](const GenLayerArgs<T>& a, bool x_fm) {
		if constexpr (Gen<T>::PRE_EPILOGUES) {
			if (keeps_pre) {
				if (x_fm) {
					gen_launch_layer<T, GEN_EPI_FORWARD_PRE, true, false>(stream, a);
				} else {
					gen_launch_layer<T, GEN_EPI_FORWARD_PRE, false, false>(stream, a);
				}
				return;
			}
		}
		if (x_fm) {
			gen_launch_layer<T, GEN_EPI_FORWARD, true, false>(stream, a);
		} else {
			gen_launch_layer<T, GEN_EPI_FORWARD, false, false>(stream, a);
		}
	};
	const T* Wl = params;
	const T* x = input;
	uint32_t K = m.in_width;
	for (uint32_t layer = 0; layer <= HM; ++layer) {
		T* y = hidden ? hidden + layer * layer_elems : ping + (layer & 1u) * layer_elems;
		hidden_layer({n, W, K, Wl, x, K, y, W, nullptr, 0u, m.activation, pre_block ? pre_block + layer * layer_elems : nullptr, nullptr, 0u, 0u, 0u, 0u},
		             layer == 0);  // the network input is feature-major
		Wl += (size_t)W * K;
		x = y;
		K = W;
	}
	GenLayerArgs<T> a = {n, m.padded_out, W, Wl, x, W, output, m.padded_out, nullptr, 0u, m.output_activation, nullptr, nullptr, 0u, 0u, 0u, 0u};
	if (trimmed.out) {
		a.Yt = trimmed.out;
		a.t_dims = trimmed.dims;
		a.t_stride_i = trimmed.stride_i;
		a.t_stride_j = trimmed.stride_j;
		a.t_vec = gen_trimmed_vec(trimmed);
		gen_launch_layer<T, GEN_EPI_FORWARD_TRIMMED, false, false>(stream, a);
	} else {
		gen_launch_layer<T, GEN_EPI_FORWARD, false, false>(stream, a);
	}
}

// The fp32 slabs of all slices may take this much scratch.  512 slabs (what the fused kernels write) of a 1024 x 4 network would be 8 GB.
constexpr size_t MLP_GENERAL_SLAB_BUDGET_BYTES = (size_t)128 << 20;
constexpr uint32_t GEN_WG_TARGET_BLOCKS = 1024;  // (tiles x slices) to aim for: four workgroups per CU
constexpr uint32_t GEN_WG_MAX_SLICES = 32;

static uint32_t gen_wgrad_tiles(uint32_t WO, uint32_t WI) { return div_round_up(WO, GEN_WG_TILE) * div_round_up(WI, GEN_WG_TILE); }

// Number of batch slices == fp32 slabs of the weight-gradient pass.  Parallelism comes from tiles x slices: as many slices as bring the
// launch of the hidden matrices to GEN_WG_TARGET_BLOCKS workgroups, at most GEN_WG_MAX_SLICES, at most one per LDS stage of samples (64
// 16-bit, 32 fp32), and no more than fit MLP_GENERAL_SLAB_BUDGET_BYTES (a single slab is always granted) -- rounded down to a power of
// two, so that the slab buffer takes few distinct sizes in the scratch cache as batch sizes vary.
template <typename T>
static uint32_t gen_n_partials(const MlpMeta& m, uint32_t n) {
	const uint32_t tiles = std::max(gen_wgrad_tiles(m.width, m.width), gen_wgrad_tiles(m.width, m.in_width));
	const size_t by_budget = MLP_GENERAL_SLAB_BUDGET_BYTES / ((size_t)m.n_params() * sizeof(float));
	uint32_t wanted = std::min(div_round_up(GEN_WG_TARGET_BLOCKS, tiles), GEN_WG_MAX_SLICES);
	wanted = std::min(wanted, std::max(n / Gen<T>::WG_BS, 1u));
	wanted = (uint32_t)std::min<size_t>(wanted, std::max<size_t>(by_budget, 1));
	uint32_t slices = 1;
	while (slices * 2u <= wanted) slices *= 2u;
	return slices;
}

template <typename T>
static size_t gen_backward_workspace_bytes(const MlpMeta& m, uint32_t n) {  // dL/d(pre-activation) of every hidden layer, [n_hidden][n][W]
	return (size_t)(m.n_hidden_matmuls + 1) * n * m.width * sizeof(T);
}

template <typename T>
static void gen_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const T* params_t, const T* input, const T* hidden, const T* dL_doutput, T* dL_dinput, float* partials,
                         void* workspace) {
	const uint32_t W = m.width, IN = m.in_width, HM = m.n_hidden_matmuls, OUTP = m.padded_out;
	const size_t layer_elems = (size_t)n * W;
	T* dact = (T*)workspace;  // [n_hidden][n][W]
	const T* wt_in = params_t;                             // [IN][W]
	const T* wt_hid = wt_in + (size_t)IN * W;              // HM x [W][W]  (row = input neuron of the matrix)
	const T* wt_out = wt_hid + (size_t)HM * W * W;         // [W][OUTP]

	// dA_last = (dY W_out) * act'(A_last), then down the hidden matrices.  The derivative is taken at the saved post-activations, or -- SiLU /
	// Sine -- at the pre-activations in the stack's second block; the weight-gradient products below read the first block either way.
	const bool keeps_pre = act_needs_preactivation(m.activation);
	const T* at = keeps_pre ? hidden + (HM + 1) * layer_elems : hidden;
	auto derivative_layer = [&](uint32_t K, const T* wt, const T* x, uint32_t j) {
		const GenLayerArgs<T> a = {n, W, K, wt, x, K, dact + j * layer_elems, W, at + j * layer_elems, W, m.activation, nullptr, nullptr, 0u, 0u, 0u, 0u};
		if constexpr (Gen<T>::PRE_EPILOGUES) {
			if (keeps_pre) return gen_launch_layer<T, GEN_EPI_BACKWARD_PRE, false, false>(stream, a);
		}
		gen_launch_layer<T, GEN_EPI_BACKWARD, false, false>(stream, a);
	};
	derivative_layer(OUTP, wt_out, dL_doutput, HM);
	for (uint32_t j = HM; j-- > 0;) derivative_layer(W, wt_hid + (size_t)j * W * W, dact + (j + 1) * layer_elems, j);
	if (dL_dinput) {  // no activation on the network input; feature-major like the input
		const GenLayerArgs<T> a = {n, IN, W, wt_in, dact, W, dL_dinput, 0u, nullptr, 0u, (uint32_t)Activation::None, nullptr, nullptr, 0u, 0u, 0u, 0u};
		gen_launch_layer<T, GEN_EPI_NONE, false, true>(stream, a);
	}
	if (!partials) return;

	const uint32_t n_slices = gen_n_partials<T>(m, n);
	const size_t slab = m.n_params(), off_hid = (size_t)W * IN, off_out = off_hid + (size_t)HM * W * W;
	const uint32_t lds_bytes = 2u * Gen<T>::WG_STAGE * (uint32_t)sizeof(T);  // 40 KiB
	auto product = [&](uint32_t WO, uint32_t WI, const T* d, uint32_t ldd, const T* a, uint32_t lda, bool a_fm, size_t offset) {
		const GenWgradArgs<T> p = {n, WO, WI, d, ldd, a, lda, partials, slab, offset, n_slices};
		const dim3 grid(gen_wgrad_tiles(WO, WI) * n_slices), block(GEN_THREADS);
		if (a_fm) {
			TCNN_LAUNCH((k_mlp_general_wgrad<T, true>), grid, block, lds_bytes, stream, p);
		} else {
			TCNN_LAUNCH((k_mlp_general_wgrad<T, false>), grid, block, lds_bytes, stream, p);
		}
	};
	product(OUTP, W, dL_doutput, OUTP, hidden + HM * layer_elems, W, false, off_out);
	for (uint32_t j = 0; j < HM; ++j) product(W, W, dact + (j + 1) * layer_elems, W, hidden + j * layer_elems, W, false, off_hid + (size_t)j * W * W);
	product(W, IN, dact, W, input, 0u, true, 0);  // the input matrix: a = the feature-major network input
}

}  // namespace tcnn_hip

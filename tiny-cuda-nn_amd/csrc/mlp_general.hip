// mlp_general.hip -- the layer-by-layer network for what the fused kernels are not built for (mlp_kernels.h mlp_layer_by_layer): hidden
// widths that are a multiple of 16 up to MLP_GENERAL_MAX_WIDTH other than 16 / 32 / 64 / 128, and -- at every width -- the hidden
// activations whose derivative needs the pre-activation (SiLU, Sine) and more than MLP_MAX_OUT_WIDTH padded outputs (up to
// MLP_GENERAL_MAX_OUT_WIDTH: the output matrix is one more M x K product, the weight-gradient tiles cover any row count).
// Stands where the reference's CutlassMLP stands (cutlass_mlp.cu:110-330: one GEMM
// with an activation epilogue per layer, one GEMM per layer for dL/d(pre-activation), one split-K GEMM per weight matrix) -- its BEHAVIOUR,
// not its tiling.  Same parameter layout, transposed scratch and boundary layouts as the fused kernels (mlp_kernels.h), so everything
// above the launchers is shared.
//
// Two kernels:
//   * k_mlp_general_layer:  Y[sample][m] = epilogue(sum_k Wm[m][k] X[sample][k]) for one matrix Wm [M][K] row-major.  Forward: Wm = a
//     layer's weights, epilogue = activation.  Backward: Wm = the TRANSPOSED weights (params_t), X = dL/d(pre-activation) of the layer
//     above, epilogue = the activation's derivative on the saved post-activation values.  SiLU / Sine (the _PRE epilogues): forward rounds
//     the accumulator to 16 bits, stores it into the stack's second block (training) and applies the activation to the rounded value;
//     backward multiplies the rounded accumulator by the rounded derivative at that saved pre-activation.  Both operands have k contiguous, so the
//     weights are the MFMA A operand and the activations the B operand straight out of [row][k] LDS tiles, and the accumulator fragment
//     (4 consecutive m for one sample) is an 8-byte store into the sample-major result.  The output layer of an inference into the caller's
//     fp32 matrix (GEN_EPI_FORWARD_F32, MlpF32Output) rounds to 16 bits like that store, widens the rounded values and stores the columns
//     below the unpadded width with the caller's strides: the bits of the padded 16-bit matrix put through trim_and_cast, without the matrix.
//     Workgroup: 4 waves, tile = (16 * NMB m) x (128 samples); wave w owns samples 32w .. 32w+31 and all NMB blocks of m
//     (2 B reads + NMB A reads per 2 * NMB MFMAs).  K runs in steps of 64 through two LDS stages: the global loads of step s + 1 are
//     issued into registers before the MFMAs of step s and written to the other stage after them -- one barrier per step.
//     Rows of 64 + 8 halves (144 bytes): the 16 rows of a 16-byte fragment read start 36 banks apart, i.e. on 16 different 4-bank
//     slots -- conflict-free.  LDS: 2 * (64 + 128) * 144 B = 54 KiB at NMB = 4 (two workgroups per CU).
//   * k_mlp_general_wgrad:  dW[o][i] = sum_s d[s][o] a[s][i] for one 64 x 64 tile of one matrix over one slice of the batch.  Both operands
//     arrive sample-major (k = the sample is the STRIDED index): they are staged as they lie, with 16-byte copies, and turned into
//     "samples in k" fragments by the hardware transpose read (lds_read_tr4).  Which sample an operand element stands for is free as
//     long as A and B agree: group g of a wave reads rows 4g .. 4g+3 and 16+4g .. 16+4g+3 of a 32-sample step, so the 8 rows a half wave
//     touches per read are consecutive, and with rows of 64 + 16 halves (40 dwords) they start 8 banks apart -- conflict-free.
//     The batch is cut into a fixed number of slices (mlp_general_n_partials); slice s writes its tiles into fp32 slab s in parameter
//     order, mlp_finalize_gradients sums the slabs in fixed order: deterministic, no floating-point atomics.
#include "mlp_kernels.h"

#if !defined(TCNN_HOST_EMU)
#include "scratch_cache.h"
#endif

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace tcnn_hip {

constexpr uint32_t GEN_THREADS = 256;
constexpr uint32_t GEN_BN = 128;           // samples per workgroup tile of k_mlp_general_layer
constexpr uint32_t GEN_BK = 64;            // k per LDS stage
constexpr uint32_t GEN_LDK = GEN_BK + 8;   // row stride (halves) of the [row][k] stages
constexpr uint32_t GEN_MAX_MB = 4;         // blocks of 16 m per workgroup tile, at most

// _PRE: the epilogues of the activations that keep their pre-activation (SiLU / Sine, activation_device.h act_forward4_pre / act_backward4_pre)
// _F32: GEN_EPI_FORWARD whose result goes to the caller's fp32 matrix (Yf ...) instead of Y
enum : uint32_t { GEN_EPI_NONE = 0, GEN_EPI_FORWARD = 1, GEN_EPI_BACKWARD = 2, GEN_EPI_FORWARD_PRE = 3, GEN_EPI_BACKWARD_PRE = 4, GEN_EPI_FORWARD_F32 = 5 };

struct GenLayerArgs {
	uint32_t n, M, K;
	const half_t* Wm;     // [M][K] row-major
	const half_t* X;      // sample-major [n][ldx], or feature-major [K][n] (X_FM)
	uint32_t ldx;
	half_t* Y;            // sample-major [n][ldy], or feature-major [M][n] (Y_FM)
	uint32_t ldy;
	const half_t* F;      // GEN_EPI_BACKWARD: the post-activation values the derivative is taken at, sample-major [n][ldf]
	uint32_t ldf;         // GEN_EPI_BACKWARD_PRE: the PRE-activation values, same layout
	uint32_t act;
	half_t* P;            // GEN_EPI_FORWARD_PRE: where the rounded pre-activations go, sample-major [n][ldy]; null: not saved (inference)
	// GEN_EPI_FORWARD_F32: element (sample i, m) with m < f_dims at Yf[i * f_stride_i + m * f_stride_j].  f_vec: floats per store the host
	// proved aligned for EVERY (sample, m = multiple of 4) -- 4 or 2 only with f_stride_j == 1 (gen_f32_vec) -- else 1
	float* Yf;
	uint32_t f_dims, f_stride_i, f_stride_j, f_vec;
};

// the 4 values of one accumulator fragment (m .. m + 3 of one sample), widened, into the caller's fp32 matrix: one 16-byte store where the host
// proved that alignment and all 4 columns exist; else 8-byte stores per existing pair where it proved that, a lone last column on its own;
// else column by column.  Nothing at or past f_dims is written.
TCNN_DEVICE void gen_store_f32(const GenLayerArgs& a, size_t sample, uint32_t m, h4 o) {
	const f4 v = f4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
	float* p = a.Yf + sample * a.f_stride_i + (size_t)m * a.f_stride_j;
	if (a.f_vec == 4u && m + 4u <= a.f_dims) {
		*(f4*)p = v;
	} else if (a.f_vec >= 2u) {
#pragma unroll
		for (uint32_t q = 0; q < 2; ++q) {
			if (m + 2u * q + 2u <= a.f_dims) {
				*(f2*)(p + 2u * q) = f2{v[2 * q], v[2 * q + 1]};
			} else if (m + 2u * q < a.f_dims) {
				p[2u * q] = v[2 * q];
			}
		}
	} else {
#pragma unroll
		for (uint32_t r = 0; r < 4; ++r)
			if (m + r < a.f_dims) p[(size_t)r * a.f_stride_j] = v[r];
	}
}

template <uint32_t NMB, uint32_t EPI, bool X_FM, bool Y_FM, bool GENERAL>
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_general_layer(const GenLayerArgs a) {
	constexpr uint32_t BM = 16 * NMB, CK = GEN_BK / 8;
	constexpr uint32_t W_CHUNKS = BM * CK, X_CHUNKS = GEN_BN * CK;
	constexpr uint32_t W_PER = (W_CHUNKS + GEN_THREADS - 1) / GEN_THREADS, X_PER = X_CHUNKS / GEN_THREADS;
	constexpr uint32_t STAGE = (BM + GEN_BN) * GEN_LDK;
	TCNN_DYN_LDS(lds_raw);
	half_t* lds = (half_t*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t n_mt = div_round_up(a.M, BM);
	const uint32_t m0 = (blockIdx.x % n_mt) * BM;           // m tiles fastest: neighbouring workgroups share their sample tile in L2
	const size_t s0 = (size_t)(blockIdx.x / n_mt) * GEN_BN;
	const uint32_t n_steps = div_round_up(a.K, GEN_BK);
	const h8 zero8 = {};

	// one K step of both operands, global -> registers.  Chunks past M or K read a valid address and are replaced by zeros (K is a
	// multiple of 16, a chunk is 8: wholly inside or outside) -- a select, not a branch around the load.
	h8 wreg[W_PER], xreg[X_PER];
	auto load = [&](uint32_t k0) {
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, kc = c % CK;
			const bool valid = c < W_CHUNKS && m0 + row < a.M && k0 + 8 * kc < a.K;
			const h8 v = *(const h8*)(a.Wm + (valid ? (size_t)(m0 + row) * a.K + k0 + 8 * kc : (size_t)0));
			wreg[q] = valid ? v : zero8;
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			if constexpr (X_FM) {  // consecutive lanes = consecutive features: the transposing 2-byte stores below fall into one row
				const uint32_t k = c % GEN_BK, sc = c / GEN_BK;
				const bool valid = k0 + k < a.K;
				const h8 v = *(const h8*)(a.X + (size_t)(valid ? k0 + k : 0u) * a.n + s0 + 8 * sc);
				xreg[q] = valid ? v : zero8;
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				const bool valid = k0 + 8 * kc < a.K;
				const h8 v = *(const h8*)(a.X + (s0 + row) * a.ldx + (valid ? k0 + 8 * kc : 0u));
				xreg[q] = valid ? v : zero8;
			}
		}
	};
	auto store = [&](half_t* stage) {
		half_t* Wt = stage;
		half_t* Xt = stage + BM * GEN_LDK;
#pragma unroll
		for (uint32_t q = 0; q < W_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, kc = c % CK;
			if (c < W_CHUNKS) *(h8*)(Wt + row * GEN_LDK + 8 * kc) = wreg[q];
		}
#pragma unroll
		for (uint32_t q = 0; q < X_PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS;
			if constexpr (X_FM) {
				const uint32_t k = c % GEN_BK, sc = c / GEN_BK;
#pragma unroll
				for (uint32_t j = 0; j < 8; ++j) Xt[(8 * sc + j) * GEN_LDK + k] = xreg[q][j];
			} else {
				const uint32_t row = c / CK, kc = c % CK;
				*(h8*)(Xt + row * GEN_LDK + 8 * kc) = xreg[q];
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
		const half_t* Wt = lds + (ks & 1u) * STAGE;
		const half_t* Xt = Wt + BM * GEN_LDK;
		const bool more = ks + 1 < n_steps;
		if (more) load((ks + 1) * GEN_BK);  // in flight while the MFMAs below run
#pragma unroll
		for (uint32_t kk = 0; kk < GEN_BK / 32; ++kk) {
			h8 bv[2];
#pragma unroll
			for (uint32_t sb = 0; sb < 2; ++sb) bv[sb] = *(const h8*)(Xt + (32 * w + 16 * sb + lr) * GEN_LDK + 32 * kk + 8 * g);
#pragma unroll
			for (uint32_t mb = 0; mb < NMB; ++mb) {
				const h8 av = *(const h8*)(Wt + (16 * mb + lr) * GEN_LDK + 32 * kk + 8 * g);
#pragma unroll
				for (uint32_t sb = 0; sb < 2; ++sb) acc[mb][sb] = mfma_16x16x32(av, bv[sb], acc[mb][sb]);
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
			h4 o;
			if constexpr (EPI == GEN_EPI_FORWARD || EPI == GEN_EPI_FORWARD_F32) {
				o = act_forward4<GENERAL>(a.act, acc[mb][sb]);
			} else if constexpr (EPI == GEN_EPI_BACKWARD) {
				const h4 fv = *(const h4*)(a.F + sample * a.ldf + m);
				o = act_backward4<GENERAL>(a.act, acc[mb][sb], fv);
			} else if constexpr (EPI == GEN_EPI_FORWARD_PRE) {
				// one launch where the reference runs a product and an element-wise pass: the rounded accumulator is the saved
				// pre-activation AND the activation's argument.  Both stores behind everything this iteration computes; it loads nothing.
				h4 pre;
				o = act_forward4_pre(a.act, acc[mb][sb], pre);
				if (valid && a.P) *(h4*)(a.P + sample * a.ldy + m) = pre;
			} else if constexpr (EPI == GEN_EPI_BACKWARD_PRE) {
				const h4 pre = *(const h4*)(a.F + sample * a.ldf + m);
				o = act_backward4_pre(a.act, acc[mb][sb], pre);
			} else {
				const f4 v = acc[mb][sb];
				o = h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
			}
			if (valid) {
				if constexpr (EPI == GEN_EPI_FORWARD_F32) {
					gen_store_f32(a, sample, m, o);
				} else if constexpr (Y_FM) {
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) a.Y[(size_t)(m + r) * a.n + sample] = o[r];
				} else {
					*(h4*)(a.Y + sample * a.ldy + m) = o;
				}
			}
		}
	}
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t GEN_WG_TILE = 64;                 // out x in tile of a workgroup
constexpr uint32_t GEN_WG_BS = 64;                   // samples per LDS stage
constexpr uint32_t GEN_WG_LDT = GEN_WG_TILE + 16;    // row stride of the sample-major stages [sample][feature]
constexpr uint32_t GEN_WG_LDF = GEN_WG_BS + 8;       // row stride of the feature-major stage [feature][sample] (the network input)
constexpr uint32_t GEN_WG_STAGE = 2 * GEN_WG_BS * GEN_WG_LDT;

struct GenWgradArgs {
	uint32_t n, WO, WI;
	const half_t* d;      // sample-major [n][ldd], WO columns used
	uint32_t ldd;
	const half_t* a;      // sample-major [n][lda], or feature-major [WI][n] (A_FM)
	uint32_t lda;
	float* partials;
	size_t slab_stride, matrix_offset;
	uint32_t n_slices;
};

// 8 "samples in k" of feature col0 + (lane & 15) out of a sample-major image: rows row0 + 4g + j and row0 + 16 + 4g + j, j < 4
TCNN_DEVICE h8 gen_tr8(const half_t* image, uint32_t row0, uint32_t col0, uint32_t ld, uint32_t lane) {
	const uint32_t i = lane & 15u, g = lane >> 4;
	const half_t* p = image + (row0 + 4u * g + (i >> 2)) * ld + col0 + 4u * (i & 3u);
	return pack8(lds_read_tr4(p), lds_read_tr4(p + 16u * ld));
}

template <bool A_FM>
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_general_wgrad(const GenWgradArgs p) {
	constexpr uint32_t T = GEN_WG_TILE, BS = GEN_WG_BS, LDT = GEN_WG_LDT, LDF = GEN_WG_LDF, CK = T / 8;
	constexpr uint32_t PER = BS * CK / GEN_THREADS;  // 16-byte chunks per thread, operand and stage
	static_assert(T * (BS / 8) == BS * CK && T * LDF <= BS * LDT, "the feature-major stage has the sample-major one's chunks and room");
	TCNN_DYN_LDS(lds_raw);
	half_t* lds = (half_t*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t wo = w >> 1, wi = w & 1u;  // this wave's 32 x 32 quarter of the tile
	const uint32_t n_ti = div_round_up(p.WI, T), n_tiles = div_round_up(p.WO, T) * n_ti;
	const uint32_t tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;
	const uint32_t o0 = (tile / n_ti) * T, i0 = (tile % n_ti) * T;
	const uint32_t n_stages = p.n / BS;
	const uint32_t t_begin = (uint32_t)((uint64_t)slice * n_stages / p.n_slices), t_end = (uint32_t)((uint64_t)(slice + 1) * n_stages / p.n_slices);
	const h8 zero8 = {};

	h8 dreg[PER], areg[PER];
	auto load = [&](uint32_t t) {
		const size_t s = (size_t)t * BS;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, cc = c % CK;
			{
				const bool valid = o0 + 8 * cc < p.WO;
				const h8 v = *(const h8*)(p.d + (s + row) * p.ldd + (valid ? o0 + 8 * cc : 0u));
				dreg[q] = valid ? v : zero8;
			}
			if constexpr (A_FM) {  // row = feature, cc = block of 8 samples
				const bool valid = i0 + row < p.WI;
				const h8 v = *(const h8*)(p.a + (size_t)(valid ? i0 + row : 0u) * p.n + s + 8 * cc);
				areg[q] = valid ? v : zero8;
			} else {
				const bool valid = i0 + 8 * cc < p.WI;
				const h8 v = *(const h8*)(p.a + (s + row) * p.lda + (valid ? i0 + 8 * cc : 0u));
				areg[q] = valid ? v : zero8;
			}
		}
	};
	auto store = [&](half_t* stage) {
		half_t* dT = stage;
		half_t* aT = stage + BS * LDT;
#pragma unroll
		for (uint32_t q = 0; q < PER; ++q) {
			const uint32_t c = tid + q * GEN_THREADS, row = c / CK, cc = c % CK;
			*(h8*)(dT + row * LDT + 8 * cc) = dreg[q];
			*(h8*)(aT + row * (A_FM ? LDF : LDT) + 8 * cc) = areg[q];
		}
	};

	f4 acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
	if (t_begin < t_end) {
		load(t_begin);
		store(lds);
	}
	__syncthreads();
	for (uint32_t t = t_begin; t < t_end; ++t) {
		const half_t* dT = lds + ((t - t_begin) & 1u) * GEN_WG_STAGE;
		const half_t* aT = dT + BS * LDT;
		const bool more = t + 1 < t_end;
		if (more) load(t + 1);
#pragma unroll
		for (uint32_t kk = 0; kk < BS / 32; ++kk) {
			h8 av[2], bv[2];
#pragma unroll
			for (uint32_t b = 0; b < 2; ++b) {
				av[b] = gen_tr8(dT, 32 * kk, 32 * wo + 16 * b, LDT, lane);
				if constexpr (A_FM) {  // samples are contiguous here: the same 4 + 4 samples per lane group, read directly
					const half_t* row = aT + (32 * wi + 16 * b + lr) * LDF + 32 * kk + 4 * g;
					bv[b] = pack8(*(const h4*)row, *(const h4*)(row + 16));
				} else {
					bv[b] = gen_tr8(aT, 32 * kk, 32 * wi + 16 * b, LDT, lane);
				}
			}
#pragma unroll
			for (uint32_t oi = 0; oi < 2; ++oi)
#pragma unroll
				for (uint32_t ii = 0; ii < 2; ++ii) acc[oi][ii] = mfma_16x16x32(av[oi], bv[ii], acc[oi][ii]);
		}
		if (more) store(lds + ((t + 1 - t_begin) & 1u) * GEN_WG_STAGE);
		__syncthreads();
	}

	// this slice's slab, parameter order; accumulator element r <-> (out = 4 g + r, in = lr) of its 16 x 16 block.  Every block inside the
	// matrix is written by every slice (zeros from a slice without samples): mlp_finalize_gradients reads all of them.
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

template <uint32_t EPI, bool X_FM, bool Y_FM>
static void gen_launch_layer(hipStream_t stream, const GenLayerArgs& a) {
	const uint32_t nmb = gen_pick_nmb(a.M);
	const dim3 grid(div_round_up(a.M, 16u * nmb) * (a.n / GEN_BN)), block(GEN_THREADS);
	const uint32_t lds_bytes = 2u * (16u * nmb + GEN_BN) * GEN_LDK * (uint32_t)sizeof(half_t);  // <= 54 KiB
	const bool general = EPI != GEN_EPI_NONE && !act_is_simple(a.act);
	// the _PRE epilogues have one instance per tile shape (GENERAL says nothing there); the other instances are what they were
#define TCNN_GEN_LAUNCH(NMB_)                                                                                                 \
	if constexpr (EPI == GEN_EPI_FORWARD_PRE || EPI == GEN_EPI_BACKWARD_PRE) {                                                \
		TCNN_LAUNCH((k_mlp_general_layer<NMB_, EPI, X_FM, Y_FM, true>), grid, block, lds_bytes, stream, a);                   \
	} else if (general) {                                                                                                     \
		TCNN_LAUNCH((k_mlp_general_layer<NMB_, EPI, X_FM, Y_FM, EPI != GEN_EPI_NONE>), grid, block, lds_bytes, stream, a);    \
	} else {                                                                                                                  \
		TCNN_LAUNCH((k_mlp_general_layer<NMB_, EPI, X_FM, Y_FM, false>), grid, block, lds_bytes, stream, a);                  \
	}
	switch (nmb) {
		case 1: TCNN_GEN_LAUNCH(1) break;
		case 2: TCNN_GEN_LAUNCH(2) break;
		case 3: TCNN_GEN_LAUNCH(3) break;
		default: TCNN_GEN_LAUNCH(4) break;
	}
#undef TCNN_GEN_LAUNCH
}

// floats per store of gen_store_f32: rows start stride_i floats apart and a fragment at a multiple of 4 columns, so with unit column
// stride a 16-byte (8-byte) store is aligned everywhere iff the base is and stride_i is a multiple of 4 (2)
static uint32_t gen_f32_vec(const MlpF32Output& f) {
	if (f.stride_j != 1u) return 1u;
	const uintptr_t base = (uintptr_t)f.out;
	if (base % 16u == 0u && f.stride_i % 4u == 0u) return 4u;
	if (base % 8u == 0u && f.stride_i % 2u == 0u) return 2u;
	return 1u;
}

void mlp_general_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const half_t* params, const half_t* input, half_t* hidden, half_t* output,
                         const MlpF32Output& f32) {
	const uint32_t W = m.width, HM = m.n_hidden_matmuls;
	if (f32.out && (hidden || output)) throw std::runtime_error("mlp_general_forward: the fp32 output is for inference, in place of the 16-bit one");
	if (f32.out && (f32.dims == 0 || f32.dims > m.padded_out)) throw std::runtime_error("mlp_general_forward: the fp32 output has at most padded_out columns");
	// inference keeps two ping-pong activation matrices [n][W] instead of the saved stack: stream-ordered scratch of this call
	const size_t layer_elems = (size_t)n * W;
	half_t* ping = nullptr;
#if defined(TCNN_HOST_EMU)
	std::vector<half_t> ping_host;
	if (!hidden) {
		ping_host.resize(2 * layer_elems);
		ping = ping_host.data();
	}
#else
	Scratch ping_scratch;
	if (!hidden) {
		ping_scratch = Scratch(stream, 2 * layer_elems * sizeof(half_t));
		ping = ping_scratch.as<half_t>();
	}
#endif
	// SiLU / Sine: the saved stack has a second block, the pre-activations (mlp_saved_activation_bytes); inference saves neither
	const bool keeps_pre = act_needs_preactivation(m.activation);
	half_t* pre_block = keeps_pre && hidden ? hidden + (HM + 1) * layer_elems : nullptr;
	const half_t* Wl = params;
	const half_t* x = input;
	uint32_t K = m.in_width;
	for (uint32_t layer = 0; layer <= HM; ++layer) {
		half_t* y = hidden ? hidden + layer * layer_elems : ping + (layer & 1u) * layer_elems;
		const GenLayerArgs a = {n, W, K, Wl, x, K, y, W, nullptr, 0u, m.activation, pre_block ? pre_block + layer * layer_elems : nullptr};
		if (keeps_pre) {
			if (layer == 0) {
				gen_launch_layer<GEN_EPI_FORWARD_PRE, true, false>(stream, a);
			} else {
				gen_launch_layer<GEN_EPI_FORWARD_PRE, false, false>(stream, a);
			}
		} else if (layer == 0) {
			gen_launch_layer<GEN_EPI_FORWARD, true, false>(stream, a);  // the network input is feature-major
		} else {
			gen_launch_layer<GEN_EPI_FORWARD, false, false>(stream, a);
		}
		Wl += (size_t)W * K;
		x = y;
		K = W;
	}
	GenLayerArgs a = {n, m.padded_out, W, Wl, x, W, output, m.padded_out, nullptr, 0u, m.output_activation, nullptr};
	if (f32.out) {
		a.Yf = f32.out;
		a.f_dims = f32.dims;
		a.f_stride_i = f32.stride_i;
		a.f_stride_j = f32.stride_j;
		a.f_vec = gen_f32_vec(f32);
		gen_launch_layer<GEN_EPI_FORWARD_F32, false, false>(stream, a);
	} else {
		gen_launch_layer<GEN_EPI_FORWARD, false, false>(stream, a);
	}
}

// The fp32 slabs of all slices may take this much scratch.  512 slabs (what the fused kernels write) of a 1024 x 4 network would be 8 GB.
constexpr size_t MLP_GENERAL_SLAB_BUDGET_BYTES = (size_t)128 << 20;
constexpr uint32_t GEN_WG_TARGET_BLOCKS = 1024;  // (tiles x slices) to aim for: four workgroups per CU
constexpr uint32_t GEN_WG_MAX_SLICES = 32;

static uint32_t gen_wgrad_tiles(uint32_t WO, uint32_t WI) { return div_round_up(WO, GEN_WG_TILE) * div_round_up(WI, GEN_WG_TILE); }

// Number of batch slices == fp32 slabs of the weight-gradient pass.  Parallelism comes from tiles x slices: as many slices as bring the
// launch of the hidden matrices to GEN_WG_TARGET_BLOCKS workgroups, at most GEN_WG_MAX_SLICES, at most one per LDS stage of samples, and no
// more than fit MLP_GENERAL_SLAB_BUDGET_BYTES (a single slab is always granted) -- rounded down to a power of two, so that the slab
// buffer takes few distinct sizes in the scratch cache as batch sizes vary.
uint32_t mlp_general_n_partials(const MlpMeta& m, uint32_t n) {
	const uint32_t tiles = std::max(gen_wgrad_tiles(m.width, m.width), gen_wgrad_tiles(m.width, m.in_width));
	const size_t by_budget = MLP_GENERAL_SLAB_BUDGET_BYTES / ((size_t)m.n_params() * sizeof(float));
	uint32_t wanted = std::min(div_round_up(GEN_WG_TARGET_BLOCKS, tiles), GEN_WG_MAX_SLICES);
	wanted = std::min(wanted, std::max(n / GEN_WG_BS, 1u));
	wanted = (uint32_t)std::min<size_t>(wanted, std::max<size_t>(by_budget, 1));
	uint32_t slices = 1;
	while (slices * 2u <= wanted) slices *= 2u;
	return slices;
}

size_t mlp_general_backward_workspace_bytes(const MlpMeta& m, uint32_t n) {  // dL/d(pre-activation) of every hidden layer, [n_hidden][n][W]
	return (size_t)(m.n_hidden_matmuls + 1) * n * m.width * sizeof(half_t);
}

void mlp_general_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const half_t* params_t, const half_t* input, const half_t* hidden,
                          const half_t* dL_doutput, half_t* dL_dinput, float* partials, void* workspace) {
	if (!workspace) throw std::runtime_error("mlp_backward: networks of this width run layer by layer and need a workspace (mlp_backward_workspace_bytes)");
	const uint32_t W = m.width, IN = m.in_width, HM = m.n_hidden_matmuls, OUTP = m.padded_out;
	const size_t layer_elems = (size_t)n * W;
	half_t* dact = (half_t*)workspace;  // [n_hidden][n][W]
	const half_t* wt_in = params_t;                             // [IN][W]
	const half_t* wt_hid = wt_in + (size_t)IN * W;              // HM x [W][W]  (row = input neuron of the matrix)
	const half_t* wt_out = wt_hid + (size_t)HM * W * W;         // [W][OUTP]

	// dA_last = (dY W_out) * act'(A_last), then down the hidden matrices.  The derivative is taken at the saved post-activations, or -- SiLU /
	// Sine -- at the pre-activations in the stack's second block; the weight-gradient products below read the first block either way.
	const bool keeps_pre = act_needs_preactivation(m.activation);
	const half_t* at = keeps_pre ? hidden + (HM + 1) * layer_elems : hidden;
	auto derivative_layer = [&](const GenLayerArgs& a) {
		if (keeps_pre) {
			gen_launch_layer<GEN_EPI_BACKWARD_PRE, false, false>(stream, a);
		} else {
			gen_launch_layer<GEN_EPI_BACKWARD, false, false>(stream, a);
		}
	};
	derivative_layer({n, W, OUTP, wt_out, dL_doutput, OUTP, dact + HM * layer_elems, W, at + HM * layer_elems, W, m.activation, nullptr});
	for (uint32_t j = HM; j-- > 0;) {
		derivative_layer({n, W, W, wt_hid + (size_t)j * W * W, dact + (j + 1) * layer_elems, W, dact + j * layer_elems, W, at + j * layer_elems, W, m.activation, nullptr});
	}
	if (dL_dinput) {  // no activation on the network input; feature-major like the input
		const GenLayerArgs a = {n, IN, W, wt_in, dact, W, dL_dinput, 0u, nullptr, 0u, (uint32_t)Activation::None, nullptr};
		gen_launch_layer<GEN_EPI_NONE, false, true>(stream, a);
	}
	if (!partials) return;

	const uint32_t n_slices = mlp_general_n_partials(m, n);
	const size_t slab = m.n_params(), off_hid = (size_t)W * IN, off_out = off_hid + (size_t)HM * W * W;
	const uint32_t lds_bytes = 2u * GEN_WG_STAGE * (uint32_t)sizeof(half_t);  // 40 KiB
	auto product = [&](uint32_t WO, uint32_t WI, const half_t* d, uint32_t ldd, const half_t* a, uint32_t lda, bool a_fm, size_t offset) {
		const GenWgradArgs p = {n, WO, WI, d, ldd, a, lda, partials, slab, offset, n_slices};
		const dim3 grid(gen_wgrad_tiles(WO, WI) * n_slices), block(GEN_THREADS);
		if (a_fm) {
			TCNN_LAUNCH((k_mlp_general_wgrad<true>), grid, block, lds_bytes, stream, p);
		} else {
			TCNN_LAUNCH((k_mlp_general_wgrad<false>), grid, block, lds_bytes, stream, p);
		}
	};
	product(OUTP, W, dL_doutput, OUTP, hidden + HM * layer_elems, W, false, off_out);
	for (uint32_t j = 0; j < HM; ++j) product(W, W, dact + (j + 1) * layer_elems, W, hidden + j * layer_elems, W, false, off_hid + (size_t)j * W * W);
	product(W, IN, dact, W, input, 0u, true, 0);  // the input matrix: a = the feature-major network input
}

}  // namespace tcnn_hip

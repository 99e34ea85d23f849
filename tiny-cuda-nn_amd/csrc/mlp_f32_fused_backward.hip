// mlp_f32_fused_backward.hip -- the fused backward pass of the fp32 network (mlp_kernels.h mlp_f32_fused_backward), two launches where the
// layer-by-layer pass (mlp_general_impl.h gen_backward) makes one per layer and one per weight matrix.  The reference has no fused fp32 network.
//
// 1. k_mlp_f32_backward_chain: dL/doutput -> D_HM .. D_0 -> dL/dinput for a tile of 256 samples.  D_j = (W_{j+1}^T D_{j+1}) * act'(at_j) is the
//    forward pass run on the transposed matrices (params_t: [IN][W] | HM x [W][W]^T | [W][OUTP]) in reverse order, so it is built on the
//    register hand-over of k_mlp_f32_fused (mlp_f32_fused.hip describes it, the split and the LDS rows of K + 8 floats): a wave owns 32 samples
//    as two 16-column tiles, column c of tile j is sample s0 + 2 c + j, the accumulator registers of D_{j+1} ARE the B operand of the next
//    product, one 16-byte LDS read of a transposed weight row feeds four MFMAs per sample tile.
//      * dL/doutput is sample-major [n][OUTP]: the lane's 16 bytes at column 16 t + 4 g of its sample are tile t in the accumulator layout; the
//        first product streams them 16 outputs at a time, the next block in flight behind the MFMAs (OUTP is a run-time count of tiles).
//      * at_j (the saved post-activations; SiLU / Sine: the pre-activation block behind them, as gen_backward chooses) is loaded as 16-byte rows
//        BEFORE the layer's MFMAs and meets the accumulators in the epilogue; act32_backward4 in place.  D_j goes to the workspace [L][n][W] as
//        16-byte rows only when weight gradients were asked for.
//      * dL/dinput is feature-major [IN][n], 16 features at a time: register r of both sample tiles is samples s0, s0 + 1 of feature
//        16 mt + 4 g + r -- one 8-byte store, 128 contiguous bytes per 16 lanes.  Without dL_dinput the input matrix is neither loaded nor used.
//    Weights resident in LDS when they fit F32F_RESIDENT_LDS_BYTES, else one matrix at a time between two barriers.
//
// 2. k_mlp_f32_wgrad_all: EVERY weight matrix in one launch.  Work item = (matrix, batch slice), matrix fastest.  The item's whole matrix (at
//    most 64 x 128) stays in accumulators for the length of its slice: 16 x 16 tiles in 2 x 2 blocks over the 8 waves (at most 2 x 4 blocks; a
//    64 x 64 matrix occupies 4 waves, a 16- or 32-wide one 1 -- the other waves still move the samples, and the kernel is bound by those
//    loads: per 32 samples a wave has at most 32 MFMAs = 1024 cycles against 8 .. 28 KiB to stage).  dW[o][i] = sum_s d[s][o] a[s][i]:
//        input matrix   d = D_0            a = the feature-major network input
//        hidden matrix  d = D_j            a = A_{j-1}, the saved post-activations
//        output matrix  d = dL/doutput     a = A_last
//    Samples stream through two LDS stages of 32: sample-major operands as they lie, rows of next_multiple(width, 32) + 16 floats, so that
//    the four rows 4 q + g of a "samples in k" read (plain 4-byte reads, column = the lane's row of the tile) start 16 banks apart; the
//    feature-major input as [feature][32 + 4].  All global loads of stage t + 1 are issued before the MFMAs of stage t and stored to the other
//    buffer after them (loads and stores share vmcnt), one barrier per stage.
//    Parts of a matrix as work items were not needed: the matrices of one network differ by at most 8 x in size, and a launch has four
//    workgroups per CU to even that out.
//    Slice s covers the sample tiles [s T / S, (s + 1) T / S) -- any T >= S -- in ascending order and writes every element of its slab
//    ([slab][n_params], parameter order) exactly once; k_mlp_f32_finalize sums the slabs in ascending order.  S = mlp_f32_fused_n_partials(m, n)
//    depends on the network and n alone, so results depend neither on the launch geometry nor on earlier calls.
//    (The kernel itself stands in mlp_f32_fused_device.h: the second-order pass instantiates it with two operand pairs.)
#include "mlp_f32_fused_device.h"

#include <algorithm>
#include <stdexcept>

namespace tcnn_hip {

struct F32ChainArgs {
	MlpMeta m;
	uint32_t n, n_tiles;
	uint32_t resident;       // every matrix has its own place in LDS (else: one buffer, staged matrix by matrix)
	const float* params_t;
	const float* at;         // [n_hidden][n][W]: where the hidden activation's derivative is taken
	const float* dL_doutput; // sample-major [n][padded_out], w.r.t. the output pre-activation
	float* dL_dinput;        // feature-major [in_width][n], or null
	float* dact;             // [n_hidden][n][W] D_j for the weight-gradient kernel, or null
};

template <uint32_t W, bool GENERAL>
__global__ void __launch_bounds__(F32F_THREADS) k_mlp_f32_backward_chain(const F32ChainArgs a) {
	constexpr uint32_t NT = W / 16u, LDW = W + F32F_PAD;
	TCNN_DYN_LDS(lds_raw);
	float* lds = (float*)lds_raw;

	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, c = lane & 15u, g = lane >> 4;
	const uint32_t IN = a.m.in_width, HM = a.m.n_hidden_matmuls, OUTP = a.m.padded_out, LDO = OUTP + F32F_PAD;
	const uint32_t act = a.m.activation;
	const size_t n = a.n, layer_elems = n * W;
	const float* wt_in = a.params_t;                       // [IN][W]
	const float* wt_hid = wt_in + (size_t)IN * W;          // HM x [W][W], row = the matrix's input neuron
	const float* wt_out = wt_hid + (size_t)HM * W * W;     // [W][OUTP]
	const bool resident = a.resident != 0u, want_dx = a.dL_dinput != nullptr;  // (uniform)
	// where each matrix lies in LDS, in the order of use
	const float* l_out = lds;
	const float* l_hid = resident ? lds + W * LDO : lds;
	const float* l_in = resident ? l_hid + HM * W * LDW : lds;
	if (resident) {
		f32f_copy_matrix(lds, wt_out, W, OUTP);
		for (uint32_t l = 0; l < HM; ++l) f32f_copy_matrix(lds + W * LDO + l * W * LDW, wt_hid + (size_t)l * W * W, W, W);
		if (want_dx) f32f_copy_matrix(lds + W * LDO + HM * W * LDW, wt_in, IN, W);
		__syncthreads();
	}
	// staged: every wave is done with the buffer's last matrix before the next one overwrites it, and sees it whole before reading
	auto stage = [&](const float* src, uint32_t rows, uint32_t K) {
		if (resident) return;
		__syncthreads();
		f32f_copy_matrix(lds, src, rows, K);
		__syncthreads();
	};

	for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {  // (uniform per workgroup: the barriers in stage() are safe)
		// this lane's column of sample tile j stands for sample s0 + j
		const size_t s0 = (size_t)tile * MLP_F32_FUSED_TILE + F32F_WAVE_SAMPLES * wave + 2u * c;

		// the values layer `layer`'s derivative is taken at: neurons 16 mt + 4 g .. + 3 of the lane's two samples, in flight during the MFMAs
		auto load_at = [&](f4 (&at)[NT][2], uint32_t layer) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt)
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) at[mt][j] = *(const f4*)(a.at + layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g);
		};
		// a finished product, in place on its accumulators: times the activation's derivative, D_j out (weight gradients asked for).  The
		// fragments are read behind branches: the MFMA wait states are spent first (mfma_settle)
		auto finish = [&](f4 (&h)[NT][2], const f4 (&at)[NT][2], uint32_t layer) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
				mfma_settle(h[mt][0]);
				mfma_settle(h[mt][1]);
			}
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) {
					h[mt][j] = act32_backward4<GENERAL>(act, h[mt][j], at[mt][j]);
					if (a.dact) *(f4*)(a.dact + layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g) = h[mt][j];
				}
			}
		};

		// ---- D_HM = (W_out^T dY) * act'(at_HM): k = the outputs, streamed in blocks of 16, the next block's loads in flight behind the MFMAs
		stage(wt_out, W, OUTP);
		f4 h[NT][2], at[NT][2];
#pragma unroll
		for (uint32_t mt = 0; mt < NT; ++mt) h[mt][0] = h[mt][1] = zero4();
		load_at(at, HM);
		{
			const float* yp = a.dL_doutput + s0 * OUTP + 4u * g;  // outputs 16 t + 4 g .. + 3 of sample s0 + j at yp[j * OUTP + 16 t]
			const uint32_t n_t = OUTP / 16u;
			f4 y[2] = {*(const f4*)yp, *(const f4*)(yp + OUTP)};
			for (uint32_t t = 0; t < n_t; ++t) {
				const uint32_t tn = t + 1u < n_t ? t + 1u : t;  // (the last block loads itself again: no branch around the loads)
				const f4 yn[2] = {*(const f4*)(yp + 16u * tn), *(const f4*)(yp + OUTP + 16u * tn)};
#pragma unroll
				for (uint32_t mt = 0; mt < NT; ++mt) {
					const f4 av = *(const f4*)(l_out + (16u * mt + c) * LDO + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						h[mt][0] = mfma_16x16x4_f32(av[r], y[0][r], h[mt][0]);
						h[mt][1] = mfma_16x16x4_f32(av[r], y[1][r], h[mt][1]);
					}
				}
				y[0] = yn[0];
				y[1] = yn[1];
			}
		}
		finish(h, at, HM);

		// ---- down the hidden matrices: register r of tile t of D_{l+1} is the B operand of the step whose A is Wt_l[m][16 t + 4 g + r]
		for (uint32_t l = HM; l-- > 0;) {
			stage(wt_hid + (size_t)l * W * W, W, W);
			const float* Wl = l_hid + (resident ? l * W * LDW : 0u);
			load_at(at, l);
			f4 o[NT][2];
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) o[mt][0] = o[mt][1] = zero4();
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t t = 0; t < NT; ++t) {
					const f4 av = *(const f4*)(Wl + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						o[mt][0] = mfma_16x16x4_f32(av[r], h[t][0][r], o[mt][0]);
						o[mt][1] = mfma_16x16x4_f32(av[r], h[t][1][r], o[mt][1]);
					}
				}
			}
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
				h[mt][0] = o[mt][0];
				h[mt][1] = o[mt][1];
			}
			finish(h, at, l);
		}

		// ---- dL/dinput = W_in^T D_0, 16 features at a time: register r of the two sample tiles is samples s0, s0 + 1 of feature 16 mt + 4 g + r
		if (want_dx) {  // (uniform)
			stage(wt_in, IN, W);
			for (uint32_t mt = 0; mt < IN / 16u; ++mt) {
				f4 o[2] = {zero4(), zero4()};
#pragma unroll
				for (uint32_t t = 0; t < NT; ++t) {
					const f4 av = *(const f4*)(l_in + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						o[0] = mfma_16x16x4_f32(av[r], h[t][0][r], o[0]);
						o[1] = mfma_16x16x4_f32(av[r], h[t][1][r], o[1]);
					}
				}
				mfma_settle(o[0]);
				mfma_settle(o[1]);
				float* xp = a.dL_dinput + (size_t)(16u * mt + 4u * g) * n + s0;
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) *(f2*)(xp + (size_t)r * n) = f2{o[0][r], o[1][r]};
			}
		}
	}
}

template <uint32_t W>
static void f32b_launch_chain(hipStream_t stream, const F32ChainArgs& a) {
	const bool want_dx = a.dL_dinput != nullptr;
	const uint32_t floats = a.resident ? f32b_resident_floats(a.m, want_dx) : f32b_staged_floats(a.m, want_dx);
	const uint32_t lds_bytes = floats * (uint32_t)sizeof(float);
	const dim3 grid(std::min(a.n_tiles, F32F_MAX_BLOCKS)), block(F32F_THREADS);
	if (!act_is_simple(a.m.activation)) {
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_backward_chain<W, true>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_backward_chain<W, true>), grid, block, lds_bytes, stream, a);
	} else {  // ReLU / None: an instance without an out-of-line call in its body
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_backward_chain<W, false>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_backward_chain<W, false>), grid, block, lds_bytes, stream, a);
	}
}

void mlp_f32_fused_backward_chain(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* at, const float* dL_doutput, float* dL_dinput,
                                  float* dact) {
	F32ChainArgs a;
	a.m = m;
	a.n = n;
	a.n_tiles = n / MLP_F32_FUSED_TILE;
	a.resident = f32b_resident_floats(m, dL_dinput != nullptr) * sizeof(float) <= F32F_RESIDENT_LDS_BYTES ? 1u : 0u;
	a.params_t = params_t;
	a.at = at;
	a.dL_doutput = dL_doutput;
	a.dL_dinput = dL_dinput;
	a.dact = dact;
	switch (m.width) {
		case 16: f32b_launch_chain<16>(stream, a); break;
		case 32: f32b_launch_chain<32>(stream, a); break;
		default: f32b_launch_chain<64>(stream, a); break;
	}
}

uint32_t mlp_f32_fused_n_partials(const MlpMeta& m, uint32_t n) {
	const size_t by_budget = MLP_GENERAL_SLAB_BUDGET_BYTES / ((size_t)m.n_params() * sizeof(float));
	uint32_t wanted = div_round_up(F32G_TARGET_BLOCKS, m.n_hidden_matmuls + 2u);
	wanted = std::min(wanted, std::max(n / MLP_F32_FUSED_TILE, 1u));
	wanted = (uint32_t)std::min<size_t>(wanted, std::max<size_t>(by_budget, 1));
	uint32_t slices = 1;
	while (slices * 2u <= wanted) slices *= 2u;
	return slices;
}

void mlp_f32_fused_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* input, const float* hidden, const float* dL_doutput,
                            float* dL_dinput, float* partials, void* workspace) {
	if (!mlp_f32_fused_backward_supported(m, n)) throw std::runtime_error("mlp_f32_fused_backward: not a shape of the fused fp32 backward kernels (mlp_f32_fused_backward_supported)");
	if (!params_t || !hidden || !dL_doutput) throw std::runtime_error("mlp_f32_fused_backward: the transposed parameters, the saved activations and dL_doutput are required");
	if (partials && (!workspace || !input)) throw std::runtime_error("mlp_f32_fused_backward: weight gradients need the workspace and the network input");
	if (!dL_dinput && !partials) return;
	const uint32_t L = m.n_hidden_matmuls + 1u;
	mlp_f32_fused_backward_chain(stream, m, n, params_t, act_needs_preactivation(m.activation) ? hidden + (size_t)L * n * m.width : hidden, dL_doutput, dL_dinput,
	                             partials ? (float*)workspace : nullptr);
	if (!partials) return;

	F32WgradArgs p;
	p.m = m;
	p.n = n;
	p.n_slices = mlp_f32_fused_n_partials(m, n);
	p.stage_floats = f32g_stage_floats(m);
	p.dact = (const float*)workspace;
	p.dL_doutput = dL_doutput;
	p.hidden = hidden;
	p.input = input;
	p.partials = partials;
	const uint32_t lds_bytes = 2u * p.stage_floats * (uint32_t)sizeof(float);  // <= 56 KiB
	TCNN_LAUNCH((k_mlp_f32_wgrad_all<F32WgradArgs>), dim3((m.n_hidden_matmuls + 2u) * p.n_slices), dim3(F32G_THREADS), lds_bytes, stream, p);
}

}  // namespace tcnn_hip

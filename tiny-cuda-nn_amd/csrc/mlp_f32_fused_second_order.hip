// mlp_f32_fused_second_order.hip -- the fused second-order pass of the fp32 network (mlp_kernels.h mlp_f32_fused_backward_backward): at most
// three launches where the layer-by-layer pass (mlp_general_fp32.hip mlp_f32_backward_backward, whose comment block defines the mathematics
// and the names used here) makes one per layer and chain and one per weight matrix, with U, T, D, E, y, g and t_out through memory between
// them.  The reference has no fused fp32 network and no second-order pass through a network at all.
//
// 1. k_mlp_f32_tangent_chain (forward weights `params`): v -> t_0 = W_0 v, u_j = t_j * act'(at_j), t_{j+1} = W_{j+1} u_j, t_out = W_out u_last
//    for a tile of 256 samples, in the geometry of k_mlp_f32_fused (mlp_f32_fused.hip: a wave owns 32 samples as two 16-column tiles, the
//    accumulators of a layer are the B operand of the next product as they lie, weight rows of K + 8 floats in LDS, resident or staged).
//    at_j arrives as 16-byte rows before the layer's MFMAs.  With an output activation the kernel also forms y = out_act(W_out a_last) from
//    the saved a_last -- its 16-byte sample-major rows are the B operand layout already -- in the SAME steps as t_out: one LDS read of a
//    row of W_out feeds the MFMAs of both products.  The epilogue of 16 outputs then has t_out, y and dy in registers and writes what
//    later steps read: dL/d(dy) = t_out * out_act'(y), g = dy * out_act'(y), c_out = dy * out_act''(y) * t_out; U_j and T_j (the raw t_j)
//    leave the hidden epilogues as 16-byte rows only where the weight gradients resp. the hidden activation's curvature need them.
//
// 2. k_mlp_f32_dual_chain (transposed weights `params_t`): BOTH reverse recurrences on the register hand-over of k_mlp_f32_backward_chain,
//        e_j = W_{j+1}^T d_{j+1},  d_j = e_j * act'(at_j),      c_j = e_j * t_j * act''(at_j) + (W_{j+1}^T c_{j+1}) * act'(at_j)
//    The two products of a layer take the same A operand: one 16-byte LDS read of a transposed weight row feeds eight MFMAs per sample
//    tile pair -- four of the d chain, four of the c chain -- where two chain launches would read it twice.  LDS reads per FLOP halve, and
//    e_j never exists outside the accumulators.  T_j and at_j are loaded before the layer's MFMAs and meet both accumulator sets in the
//    epilogue; D_j and C_j go to the workspace only where weight gradients were asked for; dL/dinput = W_0^T c_0 leaves feature-major as in
//    the backward chain.  Where the hidden activation does not curve (HIDDEN_CURVES = false: only the output one does) the c epilogue is
//    the first-order one and T is not read; where the output activation does not curve, c_out is zero: the c chain starts from zero
//    accumulators and its first product is skipped.
//    Where neither curves there is no c chain at all: the pass runs k_mlp_f32_backward_chain itself for the D_j, and dL/dinput is zeros.
//
// 3. k_mlp_f32_wgrad_all<F32WgradDualArgs> (mlp_f32_fused_device.h): per stage of 32 samples the item's accumulators take d (x) u_prev
//    (u_{-1} = v; output matrix: g (x) u_last) and then c (x) a_prev (output matrix: c_out (x) a_last), both pairs staged side by side.
//    Slices, slabs and their order as in the backward pass (mlp_f32_fused_n_partials).  Without curvature only the first pair runs.
#include "mlp_f32_fused_device.h"

#include <stdexcept>

namespace tcnn_hip {

struct F32TangentArgs {
	MlpMeta m;
	uint32_t n, n_tiles;
	uint32_t resident;      // every matrix has its own place in LDS (else: one buffer, staged layer by layer)
	const float* params;
	const float* v;         // feature-major [in_width][n]
	const float* at;        // [n_hidden][n][W]: where the hidden activation's derivative is taken
	const float* a_last;    // [n][W], given where y is needed: an output activation, and any of the three outputs below
	const float* dy;        // [n][padded_out] the caller's dL_doutput; for g and c_out
	float* U;               // [n_hidden][n][W], or null
	float* T;               // [n_hidden][n][W], or null
	float* ddy;             // [n][padded_out] dL/d(dL/doutput), or null
	float* g;               // [n][padded_out], or null
	float* c_out;           // [n][padded_out], or null (never with GENERAL == false: ReLU / None do not curve)
};

template <uint32_t W, bool GENERAL>
__global__ void __launch_bounds__(F32F_THREADS) k_mlp_f32_tangent_chain(const F32TangentArgs a) {
	constexpr uint32_t NT = W / 16u, LDW = W + F32F_PAD;
	TCNN_DYN_LDS(lds_raw);
	float* lds = (float*)lds_raw;

	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, c = lane & 15u, g = lane >> 4;
	const uint32_t IN = a.m.in_width, HM = a.m.n_hidden_matmuls, OUTP = a.m.padded_out, LDI = IN + F32F_PAD;
	const uint32_t act = a.m.activation, out_act = a.m.output_activation;
	const size_t n = a.n, layer_elems = n * W;
	const float* w_in = a.params;                        // [W][IN]
	const float* w_hid = w_in + (size_t)W * IN;           // HM x [W][W]
	const float* w_out = w_hid + (size_t)HM * W * W;      // [OUTP][W]
	const bool resident = a.resident != 0u;               // (uniform, like the three below)
	const bool want_out = a.ddy || a.g || a.c_out, want_y = a.a_last != nullptr, want_dy = a.g || a.c_out;
	const float* l_in = lds;
	const float* l_hid = resident ? lds + W * LDI : lds;
	const float* l_out = resident ? l_hid + HM * W * LDW : lds;
	if (resident) {
		f32f_copy_matrix(lds, w_in, W, IN);
		for (uint32_t l = 0; l < HM; ++l) f32f_copy_matrix(lds + W * LDI + l * W * LDW, w_hid + (size_t)l * W * W, W, W);
		if (want_out) f32f_copy_matrix(lds + W * LDI + HM * W * LDW, w_out, OUTP, W);
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
		const size_t s0 = (size_t)tile * MLP_F32_FUSED_TILE + F32F_WAVE_SAMPLES * wave + 2u * c;  // column of sample tile j: sample s0 + j

		// neurons 16 mt + 4 g .. + 3 of the lane's two samples, in flight during the MFMAs
		auto load_rows = [&](f4 (&rows)[NT][2], const float* src) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt)
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) rows[mt][j] = *(const f4*)(src + (s0 + j) * W + 16u * mt + 4u * g);
		};
		// a finished t_j, in place on its accumulators: T_j out (curvature), times the activation's derivative, U_j out (weight gradients)
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
					const size_t at_ = layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g;
					if (a.T) *(f4*)(a.T + at_) = h[mt][j];
					h[mt][j] = act32_backward4<GENERAL>(act, h[mt][j], at[mt][j]);
					if (a.U) *(f4*)(a.U + at_) = h[mt][j];
				}
			}
		};

		// ---- t_0 = W_0 v: k streamed in blocks of 16 features, the next block's loads in flight while this one's MFMAs run
		stage(w_in, W, IN);
		f4 h[NT][2], at[NT][2];
#pragma unroll
		for (uint32_t mt = 0; mt < NT; ++mt) h[mt][0] = h[mt][1] = zero4();
		load_rows(at, a.at);
		{
			const float* xp = a.v + (size_t)(4u * g) * n + s0;  // feature 16 q + 4 g + r of samples s0, s0 + 1 at xp[(16 q + r) * n]
			const uint32_t n_q = IN / 16u;
			f2 x[4];
#pragma unroll
			for (uint32_t r = 0; r < 4; ++r) x[r] = *(const f2*)(xp + (size_t)r * n);
			for (uint32_t q = 0; q < n_q; ++q) {
				f2 xn[4];
				const uint32_t qn = q + 1u < n_q ? q + 1u : q;  // (the last block loads itself again: no branch around the loads)
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) xn[r] = *(const f2*)(xp + (size_t)(16u * qn + r) * n);
#pragma unroll
				for (uint32_t mt = 0; mt < NT; ++mt) {
					const f4 av = *(const f4*)(l_in + (16u * mt + c) * LDI + 16u * q + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						h[mt][0] = mfma_16x16x4_f32(av[r], x[r][0], h[mt][0]);
						h[mt][1] = mfma_16x16x4_f32(av[r], x[r][1], h[mt][1]);
					}
				}
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) x[r] = xn[r];
			}
		}
		finish(h, at, 0u);

		// ---- t_{l+1} = W_{l+1} u_l: register r of tile t of u_l is the B operand of the step whose A is Wl[m][16 t + 4 g + r]
		for (uint32_t l = 0; l < HM; ++l) {
			stage(w_hid + (size_t)l * W * W, W, W);
			const float* Wl = l_hid + (resident ? l * W * LDW : 0u);
			load_rows(at, a.at + (l + 1u) * layer_elems);
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
			finish(h, at, l + 1u);
		}

		// ---- t_out = W_out u_last and, with an output activation, y = out_act(W_out a_last) on the same reads of W_out, 16 outputs at a time
		if (!want_out) continue;  // (uniform)
		stage(w_out, OUTP, W);
		if (want_y) load_rows(at, a.a_last);  // (at is free: a_last in its place)
		for (uint32_t mt = 0; mt < OUTP / 16u; ++mt) {
			const uint32_t col = 16u * mt + 4u * g;
			f4 dy[2] = {zero4(), zero4()};
			if (want_dy) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) dy[j] = *(const f4*)(a.dy + (s0 + j) * OUTP + col);
			}
			f4 ot[2] = {zero4(), zero4()}, oy[2] = {zero4(), zero4()};
#pragma unroll
			for (uint32_t t = 0; t < NT; ++t) {
				const f4 av = *(const f4*)(l_out + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) {
					ot[0] = mfma_16x16x4_f32(av[r], h[t][0][r], ot[0]);
					ot[1] = mfma_16x16x4_f32(av[r], h[t][1][r], ot[1]);
				}
				if (want_y) {
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						oy[0] = mfma_16x16x4_f32(av[r], at[t][0][r], oy[0]);
						oy[1] = mfma_16x16x4_f32(av[r], at[t][1][r], oy[1]);
					}
				}
			}
#pragma unroll
			for (uint32_t j = 0; j < 2; ++j) {
				mfma_settle(ot[j]);
				mfma_settle(oy[j]);
			}
#pragma unroll
			for (uint32_t j = 0; j < 2; ++j) {
				const size_t at_ = (s0 + j) * OUTP + col;
				const f4 y = act32_forward4<GENERAL>(out_act, oy[j]);  // (without an output activation nothing below reads it)
				if (a.ddy) *(f4*)(a.ddy + at_) = act32_backward4<GENERAL>(out_act, ot[j], y);
				if (a.g) *(f4*)(a.g + at_) = act32_backward4<GENERAL>(out_act, dy[j], y);
				if constexpr (GENERAL) {
					if (a.c_out) {
						f4 vt;
#pragma unroll
						for (uint32_t r = 0; r < 4; ++r) vt[r] = dy[j][r] * ot[j][r];
						*(f4*)(a.c_out + at_) = act32_second4_general(out_act, vt, y);
					}
				}
			}
		}
	}
}

template <uint32_t W>
static void f32s_launch_tangent(hipStream_t stream, const F32TangentArgs& a) {
	const uint32_t floats = a.resident ? f32f_resident_floats(a.m) : f32f_staged_floats(a.m);
	const uint32_t lds_bytes = floats * (uint32_t)sizeof(float);
	const dim3 grid(std::min(a.n_tiles, F32F_MAX_BLOCKS)), block(F32F_THREADS);
	if (!act_is_simple(a.m.activation) || !act_is_simple(a.m.output_activation)) {
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_tangent_chain<W, true>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_tangent_chain<W, true>), grid, block, lds_bytes, stream, a);
	} else {  // ReLU / None: an instance without an out-of-line call in its body
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_tangent_chain<W, false>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_tangent_chain<W, false>), grid, block, lds_bytes, stream, a);
	}
}

// ---- the two reverse chains together ----------------------------------------------------------------------------------------------------
struct F32DualChainArgs {
	MlpMeta m;
	uint32_t n, n_tiles;
	uint32_t resident;       // every matrix has its own place in LDS (else: one buffer, staged matrix by matrix)
	const float* params_t;
	const float* at;         // [n_hidden][n][W]: where the hidden activation's derivatives are taken
	const float* T;          // [n_hidden][n][W] t_j (HIDDEN_CURVES only)
	const float* g;          // sample-major [n][padded_out]: dL/d(output pre-activation)
	const float* c_out;      // sample-major [n][padded_out], or null: zero
	float* dL_dinput;        // feature-major [in_width][n], or null
	float* D;                // [n_hidden][n][W] d_j and ...
	float* C;                // ... c_j for the weight-gradient kernel, or both null
};

template <uint32_t W, bool HIDDEN_CURVES>
__global__ void __launch_bounds__(F32F_THREADS) k_mlp_f32_dual_chain(const F32DualChainArgs a) {
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
	const bool resident = a.resident != 0u, want_dx = a.dL_dinput != nullptr, has_c_out = a.c_out != nullptr;  // (uniform)
	const float* l_out = lds;
	const float* l_hid = resident ? lds + W * LDO : lds;
	const float* l_in = resident ? l_hid + HM * W * LDW : lds;
	if (resident) {
		f32f_copy_matrix(lds, wt_out, W, OUTP);
		for (uint32_t l = 0; l < HM; ++l) f32f_copy_matrix(lds + W * LDO + l * W * LDW, wt_hid + (size_t)l * W * W, W, W);
		if (want_dx) f32f_copy_matrix(lds + W * LDO + HM * W * LDW, wt_in, IN, W);
		__syncthreads();
	}
	auto stage = [&](const float* src, uint32_t rows, uint32_t K) {
		if (resident) return;
		__syncthreads();
		f32f_copy_matrix(lds, src, rows, K);
		__syncthreads();
	};

	for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {  // (uniform per workgroup: the barriers in stage() are safe)
		const size_t s0 = (size_t)tile * MLP_F32_FUSED_TILE + F32F_WAVE_SAMPLES * wave + 2u * c;  // column of sample tile j: sample s0 + j

		auto load_rows = [&](f4 (&rows)[NT][2], const float* src, uint32_t layer) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt)
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) rows[mt][j] = *(const f4*)(src + layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g);
		};
		// both finished products, in place: hd holds e_j and becomes d_j, hc holds W^T c_{j+1} and becomes c_j
		auto finish = [&](f4 (&hd)[NT][2], f4 (&hc)[NT][2], const f4 (&at)[NT][2], const f4 (&tn)[NT][2], uint32_t layer) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) {
					mfma_settle(hd[mt][j]);
					mfma_settle(hc[mt][j]);
				}
			}
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) {
					const f4 e = hd[mt][j];
					hd[mt][j] = act32_backward4<true>(act, e, at[mt][j]);
					hc[mt][j] = act32_backward4<true>(act, hc[mt][j], at[mt][j]);
					if constexpr (HIDDEN_CURVES) {
						f4 et;
#pragma unroll
						for (uint32_t r = 0; r < 4; ++r) et[r] = e[r] * tn[mt][j][r];
						const f4 second = act32_second4_general(act, et, at[mt][j]);
#pragma unroll
						for (uint32_t r = 0; r < 4; ++r) hc[mt][j][r] += second[r];
					}
					if (a.D) {
						const size_t at_ = layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g;
						*(f4*)(a.D + at_) = hd[mt][j];
						*(f4*)(a.C + at_) = hc[mt][j];
					}
				}
			}
		};

		// ---- e_HM = W_out^T g and W_out^T c_out: k = the outputs, streamed in blocks of 16, the next block's loads in flight behind the MFMAs
		stage(wt_out, W, OUTP);
		f4 hd[NT][2], hc[NT][2], at[NT][2], tn[NT][2];
#pragma unroll
		for (uint32_t mt = 0; mt < NT; ++mt) hd[mt][0] = hd[mt][1] = hc[mt][0] = hc[mt][1] = zero4();
		load_rows(at, a.at, HM);
		if constexpr (HIDDEN_CURVES) load_rows(tn, a.T, HM);
		{
			const float* gp = a.g + s0 * OUTP + 4u * g;  // outputs 16 t + 4 g .. + 3 of sample s0 + j at gp[j * OUTP + 16 t]
			const float* cp = (has_c_out ? a.c_out : a.g) + s0 * OUTP + 4u * g;  // (no c_out: loaded, not used)
			const uint32_t n_t = OUTP / 16u;
			f4 y[2] = {*(const f4*)gp, *(const f4*)(gp + OUTP)}, z[2] = {*(const f4*)cp, *(const f4*)(cp + OUTP)};
			for (uint32_t t = 0; t < n_t; ++t) {
				const uint32_t tn_ = t + 1u < n_t ? t + 1u : t;  // (the last block loads itself again: no branch around the loads)
				const f4 yn[2] = {*(const f4*)(gp + 16u * tn_), *(const f4*)(gp + OUTP + 16u * tn_)};
				const f4 zn[2] = {*(const f4*)(cp + 16u * tn_), *(const f4*)(cp + OUTP + 16u * tn_)};
#pragma unroll
				for (uint32_t mt = 0; mt < NT; ++mt) {
					const f4 av = *(const f4*)(l_out + (16u * mt + c) * LDO + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						hd[mt][0] = mfma_16x16x4_f32(av[r], y[0][r], hd[mt][0]);
						hd[mt][1] = mfma_16x16x4_f32(av[r], y[1][r], hd[mt][1]);
					}
					if (has_c_out) {
#pragma unroll
						for (uint32_t r = 0; r < 4; ++r) {
							hc[mt][0] = mfma_16x16x4_f32(av[r], z[0][r], hc[mt][0]);
							hc[mt][1] = mfma_16x16x4_f32(av[r], z[1][r], hc[mt][1]);
						}
					}
				}
				y[0] = yn[0];
				y[1] = yn[1];
				z[0] = zn[0];
				z[1] = zn[1];
			}
		}
		finish(hd, hc, at, tn, HM);

		// ---- down the hidden matrices: one read of Wt_l[m][16 t + 4 g .. + 3] is the A operand of the d chain's and the c chain's four steps
		for (uint32_t l = HM; l-- > 0;) {
			stage(wt_hid + (size_t)l * W * W, W, W);
			const float* Wl = l_hid + (resident ? l * W * LDW : 0u);
			load_rows(at, a.at, l);
			if constexpr (HIDDEN_CURVES) load_rows(tn, a.T, l);
			f4 od[NT][2], oc[NT][2];
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) od[mt][0] = od[mt][1] = oc[mt][0] = oc[mt][1] = zero4();
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t t = 0; t < NT; ++t) {
					const f4 av = *(const f4*)(Wl + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						od[mt][0] = mfma_16x16x4_f32(av[r], hd[t][0][r], od[mt][0]);
						od[mt][1] = mfma_16x16x4_f32(av[r], hd[t][1][r], od[mt][1]);
						oc[mt][0] = mfma_16x16x4_f32(av[r], hc[t][0][r], oc[mt][0]);
						oc[mt][1] = mfma_16x16x4_f32(av[r], hc[t][1][r], oc[mt][1]);
					}
				}
			}
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) {
					hd[mt][j] = od[mt][j];
					hc[mt][j] = oc[mt][j];
				}
			}
			finish(hd, hc, at, tn, l);
		}

		// ---- dL/dinput = W_in^T c_0, 16 features at a time: register r of the two sample tiles is samples s0, s0 + 1 of feature 16 mt + 4 g + r
		if (want_dx) {  // (uniform)
			stage(wt_in, IN, W);
			for (uint32_t mt = 0; mt < IN / 16u; ++mt) {
				f4 o[2] = {zero4(), zero4()};
#pragma unroll
				for (uint32_t t = 0; t < NT; ++t) {
					const f4 av = *(const f4*)(l_in + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
					for (uint32_t r = 0; r < 4; ++r) {
						o[0] = mfma_16x16x4_f32(av[r], hc[t][0][r], o[0]);
						o[1] = mfma_16x16x4_f32(av[r], hc[t][1][r], o[1]);
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
static void f32s_launch_dual_chain(hipStream_t stream, const F32DualChainArgs& a) {
	const bool want_dx = a.dL_dinput != nullptr;
	const uint32_t floats = a.resident ? f32b_resident_floats(a.m, want_dx) : f32b_staged_floats(a.m, want_dx);
	const uint32_t lds_bytes = floats * (uint32_t)sizeof(float);
	const dim3 grid(std::min(a.n_tiles, F32F_MAX_BLOCKS)), block(F32F_THREADS);
	if (a.T) {
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_dual_chain<W, true>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_dual_chain<W, true>), grid, block, lds_bytes, stream, a);
	} else {
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_dual_chain<W, false>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_dual_chain<W, false>), grid, block, lds_bytes, stream, a);
	}
}

void mlp_f32_fused_backward_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* params_t, const float* input, const float* hidden,
                                     const float* v, const float* dL_doutput, float* dL_ddLdoutput, float* dL_dinput, float* partials, void* workspace) {
	if (!mlp_f32_fused_supported(m, n)) throw std::runtime_error("mlp_f32_fused_backward_backward: not a shape of the fused fp32 kernels (mlp_f32_fused_supported)");
	if (!workspace || !hidden || !input || !v || !params) {
		throw std::runtime_error("mlp_f32_fused_backward_backward: the workspace, the saved activations, the encoded input, v and the parameters are required");
	}
	const uint32_t W = m.width, IN = m.in_width, HM = m.n_hidden_matmuls, OUTP = m.padded_out, L = HM + 1u;
	const uint32_t act = m.activation, out_act = m.output_activation, none = (uint32_t)Activation::None;
	const size_t LW = (size_t)n * W, LO = (size_t)n * OUTP;
	const bool hidden_curves = !act_second_derivative_is_zero(act), output_curves = !act_second_derivative_is_zero(out_act);
	const bool curvature = (hidden_curves || output_curves) && (partials || dL_dinput);
	const bool tangent = dL_ddLdoutput || partials || curvature, first_order = partials || curvature;
	if (first_order && (!dL_doutput || !params_t)) throw std::runtime_error("mlp_f32_fused_backward_backward: dL_doutput and the transposed parameters are required");
	auto zero_dx = [&]() {
		if (hipMemsetAsync(dL_dinput, 0, (size_t)IN * n * sizeof(float), stream) != hipSuccess) throw std::runtime_error("mlp_f32_fused_backward_backward: memset failed");
	};
	if (!tangent) {
		if (dL_dinput) zero_dx();
		return;
	}

	// the workspace as the layer-by-layer pass lays it out (mlp_f32_backward_backward_workspace_bytes); y and t_out never reach it
	float* U = (float*)workspace;   // [L][n][W]
	float* D = U + L * LW;          // [L][n][W]
	float* g_buf = D + L * LW + LO; // [n][OUTP]
	float* T = g_buf + LO;          // [L][n][W]      (curvature only, like the two below)
	float* C = T + L * LW;          // [L][n][W]
	float* c_out = C + L * LW;      // [n][OUTP]
	const float* at = act_needs_preactivation(act) ? hidden + L * LW : hidden;
	const float* a_last = hidden + HM * LW;
	const uint32_t n_tiles = n / MLP_F32_FUSED_TILE;
	const float* g = first_order && out_act != none ? g_buf : dL_doutput;

	F32TangentArgs t;
	t.m = m;
	t.n = n;
	t.n_tiles = n_tiles;
	t.resident = f32f_resident_floats(m) * sizeof(float) <= F32F_RESIDENT_LDS_BYTES ? 1u : 0u;
	t.params = params;
	t.v = v;
	t.at = at;
	t.dy = dL_doutput;
	t.U = partials ? U : nullptr;
	t.T = curvature && hidden_curves ? T : nullptr;
	t.ddy = dL_ddLdoutput;
	t.g = first_order && out_act != none ? g_buf : nullptr;
	t.c_out = curvature && output_curves ? c_out : nullptr;
	t.a_last = out_act != none && (t.ddy || t.g || t.c_out) ? a_last : nullptr;
	switch (W) {
		case 16: f32s_launch_tangent<16>(stream, t); break;
		case 32: f32s_launch_tangent<32>(stream, t); break;
		default: f32s_launch_tangent<64>(stream, t); break;
	}

	if (curvature) {
		F32DualChainArgs a;
		a.m = m;
		a.n = n;
		a.n_tiles = n_tiles;
		a.resident = f32b_resident_floats(m, dL_dinput != nullptr) * sizeof(float) <= F32F_RESIDENT_LDS_BYTES ? 1u : 0u;
		a.params_t = params_t;
		a.at = at;
		a.T = t.T;
		a.g = g;
		a.c_out = t.c_out;
		a.dL_dinput = dL_dinput;
		a.D = partials ? D : nullptr;
		a.C = partials ? C : nullptr;
		switch (W) {
			case 16: f32s_launch_dual_chain<16>(stream, a); break;
			case 32: f32s_launch_dual_chain<32>(stream, a); break;
			default: f32s_launch_dual_chain<64>(stream, a); break;
		}
	} else {
		if (partials) mlp_f32_fused_backward_chain(stream, m, n, params_t, at, g, nullptr, D);
		if (dL_dinput) zero_dx();
	}
	if (!partials) return;

	F32WgradDualArgs p;
	p.m = m;
	p.n = n;
	p.n_slices = mlp_f32_fused_n_partials(m, n);
	p.stage_floats = (curvature ? 2u : 1u) * f32g_stage_floats(m);
	p.dact = D;
	p.dL_doutput = g;
	p.hidden = U;
	p.input = v;
	p.partials = partials;
	p.dact2 = curvature ? C : nullptr;
	p.dL_doutput2 = t.c_out;
	p.hidden2 = hidden;
	p.input2 = input;
	const uint32_t lds_bytes = 2u * p.stage_floats * (uint32_t)sizeof(float);  // <= 112 KiB
	TCNN_SET_MAX_DYN_LDS((k_mlp_f32_wgrad_all<F32WgradDualArgs>), lds_bytes);
	TCNN_LAUNCH((k_mlp_f32_wgrad_all<F32WgradDualArgs>), dim3((HM + 2u) * p.n_slices), dim3(F32G_THREADS), lds_bytes, stream, p);
}

}  // namespace tcnn_hip

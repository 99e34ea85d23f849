// mlp_f32_fused.hip -- the fused forward / inference kernel of the fp32 network (mlp_kernels.h mlp_f32_fused_forward): one launch carries a
// tile of samples through EVERY layer on v_mfma_f32_16x16x4_f32, and hidden activations never leave the registers except as the saved stack
// a training forward pass was asked for.  Not a port of the 16-bit wave kernel (mlp_train_wave.hip keeps activations sample-major in LDS
// tiles and weights in registers); the reference has no fused fp32 network.
//
// The hand-over the kernel is built on.  With H = W X as [neuron][sample], lane l = 16 g + c of a 16 x 16 accumulator tile holds neurons
// 4 g + r (register r = 0..3) of sample column c.  A B operand of one k-step wants lane l to hold k-slot g of column c, and the sum over k may
// run in any order: so register r of neuron tile t IS the B operand of the k-step whose four k are neurons 16 t + {r, 4 + r, 8 + r, 12 + r},
// provided that step's A operand is Wnext[m][16 t + 4 g + r].  For r = 0..3 those are four consecutive floats of a weight row: ONE 16-byte
// LDS read per lane feeds four MFMAs per sample tile.  No LDS round trip of activations, no cross-lane moves; the activation is applied in
// place on the accumulator registers.
//
// Split.  Workgroup = 8 waves (512 threads) = one tile of 256 samples, the batch granularity; a wave owns 32 samples as two 16-column tiles,
// so every weight fragment read from LDS is used by 8 MFMAs and a layer has 2 * W / 16 independent accumulator chains.  Column c of sample
// tile j stands for sample s0 + 2 c + j (which sample a column stands for is free): the feature-major network input [in_width][n] then
// arrives as one 8-byte load per lane and feature -- 128 contiguous bytes per 16 lanes -- holding the lane's column of BOTH sample tiles, and
// the lane loads features 16 q + 4 g + r, r = 0..3: the input is put into registers in the accumulator layout, so the first layer runs the
// same steps as every other one, its k-loop streamed 16 features at a time (one block in flight ahead of the MFMAs; any input width).
// Results leave as whole 16-byte rows: a lane holds 4 consecutive neurons (outputs) of a sample, i.e. 16 contiguous bytes of a sample-major
// row, and the four lanes g = 0..3 of a column cover 64 contiguous bytes of it.
// Workgroups are persistent (grid-stride over the tiles): the weights go to LDS once per workgroup.
//
// Weights in LDS: each matrix [rows][K] row-major as in the parameter vector, rows K + 8 floats apart.  A lane reads 16 bytes of row 16 mt + c
// at column 16 t + 4 g.  The 16 lanes the hardware serves together in a 16-byte read mix two values of g (lanes 0-3, 12-15, 20-27, ...), so
// the row stride has to separate rows AND the 4-float step between lane groups: with K + 8 (8 banks a row, K a multiple of 16) the 16 lanes
// of every group fall on 16 different 4-bank slots of the 64 banks -- 4 cycles per read, the ideal, at every supported K; K + 4, which
// separates the rows alone, models at 8 (scripts/lds_bank_model.py).
// All matrices resident when they fit F32F_RESIDENT_LDS_BYTES (every network of up to 5 hidden layers at 64 neurons, 128 inputs and 64 outputs, deeper
// ones at smaller widths); a deeper network stages one matrix at a time in a buffer of the largest, between two barriers per layer.
#include "mlp_f32_fused_device.h"

#include <algorithm>
#include <stdexcept>

namespace tcnn_hip {

struct F32FusedArgs {
	MlpMeta m;
	uint32_t n, n_tiles;
	uint32_t resident;      // every matrix has its own place in LDS (else: one buffer, staged layer by layer)
	const float* params;
	const float* input;     // feature-major [in_width][n]
	float* hidden;          // [n_hidden][n][W] post-activations, or null (inference)
	float* pre;             // [n_hidden][n][W] pre-activations (SiLU / Sine, training), or null
	float* output;          // sample-major [n][padded_out], or null (trimmed)
	MlpF32Output t;         // t.out given: element (i, j < dims) at out[i * stride_i + j * stride_j], nothing else written
	uint32_t t_vec;         // 4: every (sample, multiple-of-4 column) of t is 16-byte aligned with unit column stride; else 1
};

template <uint32_t W, bool GENERAL>
__global__ void __launch_bounds__(F32F_THREADS) k_mlp_f32_fused(const F32FusedArgs a) {
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
	const bool resident = a.resident != 0u;               // (uniform)
	// where each matrix lies in LDS
	const float* l_in = lds;
	const float* l_hid = resident ? lds + W * LDI : lds;
	const float* l_out = resident ? l_hid + HM * W * LDW : lds;
	if (resident) {
		f32f_copy_matrix(lds, w_in, W, IN);
		for (uint32_t l = 0; l < HM; ++l) f32f_copy_matrix(lds + W * LDI + l * W * LDW, w_hid + (size_t)l * W * W, W, W);
		f32f_copy_matrix(lds + W * LDI + HM * W * LDW, w_out, OUTP, W);
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

		// a finished hidden layer, in place on its accumulators: pre-activations out (SiLU / Sine, training), the activation,
		// post-activations out (training).  The fragments are read behind branches: the MFMA wait states are spent first (mfma_settle)
		auto finish_hidden = [&](f4 (&h)[NT][2], uint32_t layer) {
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
				mfma_settle(h[mt][0]);
				mfma_settle(h[mt][1]);
			}
#pragma unroll
			for (uint32_t mt = 0; mt < NT; ++mt) {
#pragma unroll
				for (uint32_t j = 0; j < 2; ++j) {
					const size_t at = layer * layer_elems + (s0 + j) * W + 16u * mt + 4u * g;
					if (a.pre) *(f4*)(a.pre + at) = h[mt][j];
					h[mt][j] = act32_forward4<GENERAL>(act, h[mt][j]);
					if (a.hidden) *(f4*)(a.hidden + at) = h[mt][j];
				}
			}
		};

		// ---- the input layer: k streamed in blocks of 16 features, the next block's loads in flight while this one's MFMAs run
		stage(w_in, W, IN);
		f4 h[NT][2];
#pragma unroll
		for (uint32_t mt = 0; mt < NT; ++mt) h[mt][0] = h[mt][1] = zero4();
		{
			const float* xp = a.input + (size_t)(4u * g) * n + s0;  // feature 16 q + 4 g + r of samples s0, s0 + 1 at xp[(16 q + r) * n]
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
		finish_hidden(h, 0u);

		// ---- the hidden matrices: register r of tile t of the layer below is the B operand of the step whose A is Wl[m][16 t + 4 g + r]
		for (uint32_t l = 0; l < HM; ++l) {
			stage(w_hid + (size_t)l * W * W, W, W);
			const float* Wl = l_hid + (resident ? l * W * LDW : 0u);
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
			finish_hidden(h, l + 1u);
		}

		// ---- the output layer, 16 outputs at a time: outputs 16 mt + 4 g .. + 3 of a sample are 16 contiguous bytes of its row
		stage(w_out, OUTP, W);
		for (uint32_t mt = 0; mt < OUTP / 16u; ++mt) {
			f4 o[2] = {zero4(), zero4()};
#pragma unroll
			for (uint32_t t = 0; t < NT; ++t) {
				const f4 av = *(const f4*)(l_out + (16u * mt + c) * LDW + 16u * t + 4u * g);
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) {
					o[0] = mfma_16x16x4_f32(av[r], h[t][0][r], o[0]);
					o[1] = mfma_16x16x4_f32(av[r], h[t][1][r], o[1]);
				}
			}
			mfma_settle(o[0]);
			mfma_settle(o[1]);
			const uint32_t col = 16u * mt + 4u * g;
#pragma unroll
			for (uint32_t j = 0; j < 2; ++j) {
				const f4 y = act32_forward4<GENERAL>(out_act, o[j]);
				if (a.output) {
					*(f4*)(a.output + (s0 + j) * OUTP + col) = y;
				} else {  // the caller's trimmed matrix: nothing at or past t.dims is written
					float* p = a.t.out + (s0 + j) * a.t.stride_i + (size_t)col * a.t.stride_j;
					if (a.t_vec == 4u && col + 4u <= a.t.dims) {
						*(f4*)p = y;
					} else {
#pragma unroll
						for (uint32_t r = 0; r < 4; ++r)
							if (col + r < a.t.dims) p[(size_t)r * a.t.stride_j] = y[r];
					}
				}
			}
		}
	}
}

template <uint32_t W>
static void f32f_launch(hipStream_t stream, const F32FusedArgs& a) {
	const uint32_t floats = a.resident ? f32f_resident_floats(a.m) : f32f_staged_floats(a.m);
	const uint32_t lds_bytes = floats * (uint32_t)sizeof(float);
	const dim3 grid(std::min(a.n_tiles, F32F_MAX_BLOCKS)), block(F32F_THREADS);
	if (!act_is_simple(a.m.activation) || !act_is_simple(a.m.output_activation)) {
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_fused<W, true>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_fused<W, true>), grid, block, lds_bytes, stream, a);
	} else {  // ReLU / None: an instance without an out-of-line call in its body
		TCNN_SET_MAX_DYN_LDS((k_mlp_f32_fused<W, false>), lds_bytes);
		TCNN_LAUNCH((k_mlp_f32_fused<W, false>), grid, block, lds_bytes, stream, a);
	}
}

void mlp_f32_fused_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* input, float* hidden, float* output,
                           const MlpF32Output& trimmed) {
	if (!mlp_f32_fused_supported(m, n)) throw std::runtime_error("mlp_f32_fused_forward: not a shape of the fused fp32 kernel (mlp_f32_fused_supported)");
	if (trimmed.out && (hidden || output)) throw std::runtime_error("mlp_f32_fused_forward: the trimmed output is for inference, in place of the padded one");
	if (trimmed.out && (trimmed.dims == 0 || trimmed.dims > m.padded_out)) throw std::runtime_error("mlp_f32_fused_forward: the trimmed output has at most padded_out columns");
	if (!trimmed.out && !output) throw std::runtime_error("mlp_f32_fused_forward: no output matrix");
	F32FusedArgs a;
	a.m = m;
	a.n = n;
	a.n_tiles = n / MLP_F32_FUSED_TILE;
	a.resident = f32f_resident_floats(m) * sizeof(float) <= F32F_RESIDENT_LDS_BYTES ? 1u : 0u;
	a.params = params;
	a.input = input;
	a.hidden = hidden;
	a.pre = hidden && act_needs_preactivation(m.activation) ? hidden + (size_t)(m.n_hidden_matmuls + 1u) * n * m.width : nullptr;
	a.output = output;
	a.t = trimmed;
	a.t_vec = trimmed.out && trimmed.stride_j == 1u && (uintptr_t)trimmed.out % 16u == 0u && trimmed.stride_i % 4u == 0u ? 4u : 1u;
	switch (m.width) {
		case 16: f32f_launch<16>(stream, a); break;
		case 32: f32f_launch<32>(stream, a); break;
		default: f32f_launch<64>(stream, a); break;
	}
}

}  // namespace tcnn_hip

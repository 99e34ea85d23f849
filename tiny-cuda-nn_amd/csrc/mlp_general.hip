// mlp_general.hip -- the 16-bit layer-by-layer network: Gen<half_t> and the entry points over the templates of mlp_general_impl.h, which
// describes the kernels.  (The host emulator gets this unit through mlp_kernels.hip's unity include.)
#include "mlp_general_impl.h"

namespace tcnn_hip {

template <>
struct Gen<half_t> : GenTile<half_t> {
	typedef h8 vec;      // a 16-byte chunk
	typedef h4 frag;     // the 4 values of an accumulator fragment as they are stored
	typedef h8 operand;  // one lane's share of an MFMA operand: 8 k of the 16x16x32 shape
	static constexpr uint32_t MFMA_K = 32;
	static constexpr bool PRE_EPILOGUES = true;  // SiLU / Sine have epilogues of their own (_PRE), one instance per tile shape
	// the zero chunk that replaces a load past an edge.  A compile-time constant here and a function's result in fp32: hipcc turns the first into
	// selects behind the loads and the second into branches around them, and each precision keeps the form it was tuned and measured with
	static constexpr vec zero() { return vec{}; }
	static TCNN_DEVICE operand part(vec v, uint32_t) { return v; }
	static TCNN_DEVICE f4 mfma(operand a, operand b, f4 c) { return mfma_16x16x32(a, b, c); }
	// "samples in k" for step q of a stage (samples 32 q .. 32 q + 31), feature 32 wv + 16 b + lr, wv = the wave's half of the tile.  Out of a
	// sample-major image: rows 32 q + 4g + j and 32 q + 16 + 4g + j, j < 4, through the transpose read; out of a feature-major one, where samples
	// are contiguous, the same 4 + 4 samples read directly.  (The index expressions are written term by term as they always were: hipcc's
	// address arithmetic follows their association.)
	static TCNN_DEVICE operand wg_samples(const half_t* image, uint32_t q, uint32_t wv, uint32_t b, uint32_t ld, uint32_t lane, uint32_t, uint32_t) {
		const uint32_t row0 = 32 * q, col0 = 32 * wv + 16 * b, i = lane & 15u, g = lane >> 4;
		const half_t* p = image + (row0 + 4u * g + (i >> 2)) * ld + col0 + 4u * (i & 3u);
		return pack8(lds_read_tr4(p), lds_read_tr4(p + 16u * ld));
	}
	static TCNN_DEVICE operand wg_samples_fm(const half_t* image, uint32_t q, uint32_t wv, uint32_t b, uint32_t ld, uint32_t, uint32_t lr, uint32_t g) {
		const half_t* row = image + (32 * wv + 16 * b + lr) * ld + 32 * q + 4 * g;
		return pack8(*(const h4*)row, *(const h4*)(row + 16));
	}
	template <bool GENERAL>
	static TCNN_DEVICE frag forward(uint32_t act, f4 x) { return act_forward4<GENERAL>(act, x); }
	template <bool GENERAL>
	static TCNN_DEVICE frag backward(uint32_t act, f4 v, frag at) { return act_backward4<GENERAL>(act, v, at); }
	static TCNN_DEVICE frag narrow(f4 v) { return h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]}; }
	static TCNN_DEVICE f4 widen(frag o) { return f4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]}; }
};

// ---- the 16-bit entry points (mlp_kernels.hip routes here; its check_meta holds the shape checks) -------------------------------------
void mlp_general_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const half_t* params, const half_t* input, half_t* hidden, half_t* output,
                         const MlpF32Output& f32) {
	if (f32.out && (hidden || output)) throw std::runtime_error("mlp_general_forward: the fp32 output is for inference, in place of the 16-bit one");
	if (f32.out && (f32.dims == 0 || f32.dims > m.padded_out)) throw std::runtime_error("mlp_general_forward: the fp32 output has at most padded_out columns");
	gen_forward<half_t>(stream, m, n, params, input, hidden, output, f32);
}
uint32_t mlp_general_n_partials(const MlpMeta& m, uint32_t n) { return gen_n_partials<half_t>(m, n); }
size_t mlp_general_backward_workspace_bytes(const MlpMeta& m, uint32_t n) { return gen_backward_workspace_bytes<half_t>(m, n); }
void mlp_general_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const half_t* params_t, const half_t* input, const half_t* hidden,
                          const half_t* dL_doutput, half_t* dL_dinput, float* partials, void* workspace) {
	if (!workspace) throw std::runtime_error("mlp_backward: networks of this width run layer by layer and need a workspace (mlp_backward_workspace_bytes)");
	gen_backward<half_t>(stream, m, n, params_t, input, hidden, dL_doutput, dL_dinput, partials, workspace);
}

}  // namespace tcnn_hip

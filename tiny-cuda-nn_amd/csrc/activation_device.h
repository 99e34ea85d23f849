// activation_device.h -- the activations FullyFusedMLP offers for its hidden layers (fully_fused_mlp.cu:690-697) and,
// together with None, for the output layer; reference arithmetic: common_device.h:108-186 (forward) and :363-418
// (backward, expressed through the POST-activation value -- which is all that the fused kernels store).
// SiLU and Sine (common_device.h:131-152 forward, :253-277 backward) have a derivative that needs the PRE-activation: only the
// layer-by-layer network (mlp_general.hip) offers them, as hidden activations, through act_forward4_pre / act_backward4_pre below and a saved
// stack with a second block (mlp_kernels.h mlp_saved_activation_bytes).  No other 16-bit function of this file is entered with them.
// The fp32 network's activations (act32_*, all ten in one pair of bodies, nothing rounded) are at the end.
#pragma once
#include "tcnn_device.h"
#if defined(TCNN_HOST_EMU)
#include <math.h>
#endif

namespace tcnn_hip {

enum class Activation : int { None = 0, ReLU = 1, LeakyReLU = 2, Exponential = 3, Sigmoid = 4, Squareplus = 5, Softplus = 6, Tanh = 7, SiLU = 8, Sine = 9 };  // 0-7: the oracle's ORC_ACT_* numbering
constexpr float K_ACT = 10.0f;  // common_device.h:108

// The fused kernels evaluate activations at dozens of unrolled sites: ReLU / None stay inline, everything else is ONE
// out-of-line copy (inlining the transcendental bodies everywhere doubled the training kernel's run time through
// instruction-cache misses).
#if defined(TCNN_HOST_EMU)
#define TCNN_DEVICE_NOINLINE inline
#else
#define TCNN_DEVICE_NOINLINE __device__ __attribute__((noinline))
#endif

// activation of a pre-activation accumulator (fp32); the caller rounds the result to fp16 once
TCNN_DEVICE_NOINLINE float act_forward_general(uint32_t act, float x) {
	switch ((Activation)act) {
		case Activation::ReLU: return x > 0.0f ? x : 0.0f;
		case Activation::LeakyReLU: return x * (x > 0.0f ? 1.0f : (float)(half_t)0.01f);  // common_device.h:127: the slope is a (T) constant
		case Activation::Exponential: return expf(x);
		case Activation::Sigmoid: return 1.0f / (1.0f + expf(-x));
		case Activation::Squareplus: {
			const float y = x * K_ACT;
			return 0.5f * (y + sqrtf(y * y + 4.0f)) / K_ACT;
		}
		case Activation::Softplus: return logf(expf(x * K_ACT) + 1.0f) / K_ACT;
		case Activation::Tanh: return tanhf(x);
		default: return x;
	}
}

// GENERAL == false: the kernel instance only ever sees ReLU / None (no call sites at all in its body)
template <bool GENERAL>
TCNN_DEVICE float act_forward(uint32_t act, float x) {
	if (act == (uint32_t)Activation::ReLU) return x > 0.0f ? x : 0.0f;
	if constexpr (GENERAL) {
		if (act != (uint32_t)Activation::None) return act_forward_general(act, x);
	}
	return x;
}
TCNN_HOST_DEVICE bool act_is_simple(uint32_t act) { return act == (uint32_t)Activation::ReLU || act == (uint32_t)Activation::None; }
// the derivative cannot be written through the post-activation value (sin is not monotonic; x * logistic(x) neither)
TCNN_HOST_DEVICE bool act_needs_preactivation(uint32_t act) { return act == (uint32_t)Activation::SiLU || act == (uint32_t)Activation::Sine; }

// dL/d(pre-activation) = v * f'(x) with f' written in terms of the stored fp16 post-activation value; the factor is
// rounded to fp16 like the reference's (T)(...) before the multiply.  ReLU keeps the select form (exact, no -0).
TCNN_DEVICE_NOINLINE float act_backward_general(uint32_t act, float v, half_t forward_value) {
	const float y = (float)forward_value;
	float factor;
	switch ((Activation)act) {
		case Activation::ReLU: return forward_value > (half_t)0.0f ? v : 0.0f;
		case Activation::LeakyReLU: factor = forward_value > (half_t)0.0f ? 1.0f : 0.01f; break;
		case Activation::Exponential: factor = y; break;
		case Activation::Sigmoid: factor = (float)(half_t)(y * (float)(half_t)(1.0f - y)); break;  // common_device.h:389
		case Activation::Squareplus: {
			const float t = y * K_ACT;
			factor = t * t / (t * t + 1.0f);
			break;
		}
		case Activation::Softplus: factor = 1.0f - expf(-y * K_ACT); break;
		case Activation::Tanh: factor = 1.0f - y * y; break;
		default: return v;
	}
	return v * (float)(half_t)factor;
}

// An MFMA result that is about to be read on the far side of a branch: hipcc pads the wait states between an MFMA and the first reader of its
// result in straight-line code, but can miss them on a path that leaves the MFMA through a TAKEN branch (scripts/check_mfma_branch_hazard.py,
// profiles/r03_mfma_branch_hazard.txt: stale accumulators, no fault, no message).  This spends the wait states (12 >= the 8-pass shapes' need)
// in front of the branch, tied to the fragment so that it cannot move above the MFMA.
TCNN_DEVICE void mfma_settle(f4& fragment) {
#if !defined(TCNN_HOST_EMU)
	// (between scheduling barriers: the wait states have to stand directly in front of the branch -- tied to the fragment alone, the scheduler
	// moved independent MFMAs of the surrounding loop between them and the branch)
	__builtin_amdgcn_sched_barrier(0);
	asm volatile("s_nop 7\n\ts_nop 3" : "+v"(fragment));
	__builtin_amdgcn_sched_barrier(0);
#endif
}

// ---- four values at a time: what every call site of the fused kernels has in hand (an MFMA accumulator fragment).  The out-of-line body is
// entered ONCE per fragment with the switch outside the four evaluations: per-element calls cost the 128 x 4 Sigmoid network 0.45 ms of
// call overhead and spills around the calls per step (0.667 against 0.218 ms with ReLU; scripts/exp_spilling_instances.py, round 5).
// Same arithmetic per element as the scalar forms above, same rounding points.
TCNN_DEVICE_NOINLINE f4 act_forward4_general(uint32_t act, f4 x) {
	f4 y;
	switch ((Activation)act) {
		case Activation::LeakyReLU:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] * (x[j] > 0.0f ? 1.0f : (float)(half_t)0.01f);
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
		case Activation::ReLU:
#pragma unroll
			for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] > 0.0f ? x[j] : 0.0f;
			break;
		default: y = x; break;
	}
	return y;
}
// activation of an accumulator fragment, rounded to the 16-bit type once per value
template <bool GENERAL>
TCNN_DEVICE h4 act_forward4(uint32_t act, f4 x) {
	if constexpr (GENERAL) {
		mfma_settle(x);  // the fragment is read on both sides of the branch below
		if (act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU) x = act_forward4_general(act, x);
	}
	// ReLU as a SELECT on a uniform flag, not as a branch around four selects: these fragments come straight out of an MFMA, and a taken
	// branch between an MFMA and the first reader of its result is where hipcc under-pads the wait states
	// (scripts/check_mfma_branch_hazard.py, profiles/r03_mfma_branch_hazard.txt)
	const bool relu = act == (uint32_t)Activation::ReLU;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) x[j] = (relu && !(x[j] > 0.0f)) ? 0.0f : x[j];
	return h4{(half_t)x[0], (half_t)x[1], (half_t)x[2], (half_t)x[3]};
}
TCNN_DEVICE_NOINLINE f4 act_backward4_general(uint32_t act, f4 v, h4 forward_value) {
	f4 out;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) {
		const float y = (float)forward_value[j];
		float factor = 1.0f;
		bool plain = false;
		switch ((Activation)act) {  // (uniform: the compiler hoists it out of the unrolled loop)
			case Activation::ReLU: out[j] = forward_value[j] > (half_t)0.0f ? v[j] : 0.0f; plain = true; break;
			case Activation::LeakyReLU: factor = forward_value[j] > (half_t)0.0f ? 1.0f : 0.01f; break;
			case Activation::Exponential: factor = y; break;
			case Activation::Sigmoid: factor = (float)(half_t)(y * (float)(half_t)(1.0f - y)); break;
			case Activation::Squareplus: {
				const float t = y * K_ACT;
				factor = t * t / (t * t + 1.0f);
				break;
			}
			case Activation::Softplus: factor = 1.0f - expf(-y * K_ACT); break;
			case Activation::Tanh: factor = 1.0f - y * y; break;
			default: out[j] = v[j]; plain = true; break;
		}
		if (!plain) out[j] = v[j] * (float)(half_t)factor;
	}
	return out;
}
template <bool GENERAL>
TCNN_DEVICE h4 act_backward4(uint32_t act, f4 v, h4 forward_value) {
	if constexpr (GENERAL) {
		mfma_settle(v);
		if (act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU) v = act_backward4_general(act, v, forward_value);
	}
	const bool relu = act == (uint32_t)Activation::ReLU;  // (a select, see act_forward4)
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) v[j] = (relu && !(forward_value[j] > (half_t)0.0f)) ? 0.0f : v[j];
	return h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
}

// ---- SiLU / Sine: the activations that keep their pre-activation.  The arithmetic is the reference's two-pass form (a product written as a
// 16-bit matrix, then an element-wise pass over it): the accumulator is rounded to the 16-bit type FIRST, the activation is evaluated in fp32
// on the rounded value and rounded once more; backward, the rounded accumulator is multiplied by the derivative at the saved pre-activation,
// itself rounded -- a 16-bit x 16-bit product with one rounding (exact in fp32 before it: 11 + 11 or 8 + 8 significant bits).
// The accurate sinf / cosf, not the hardware's v_sin_f32 / v_cos_f32: the first layer of a SIREN network has pre-activations of tens of
// radians, where the fast forms lose digits (their argument reduction is a multiply by 1 / 2 pi in fp32).  Same shape as the functions above:
// ONE out-of-line body per kernel, entered once per fragment, mfma_settle in front of the branch into it.
TCNN_DEVICE_NOINLINE f4 act_forward4_pre_general(uint32_t act, f4 x) {
	f4 y;
	if (act == (uint32_t)Activation::Sine) {
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) y[j] = sinf(x[j]);
	} else {  // SiLU
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) y[j] = x[j] * (1.0f / (1.0f + expf(-x[j])));
	}
	return y;
}
// accumulator fragment -> `pre` (what a training pass saves) and the activation of `pre`
TCNN_DEVICE h4 act_forward4_pre(uint32_t act, f4 x, h4& pre) {
	mfma_settle(x);
	pre = h4{(half_t)x[0], (half_t)x[1], (half_t)x[2], (half_t)x[3]};
	const f4 y = act_forward4_pre_general(act, f4{(float)pre[0], (float)pre[1], (float)pre[2], (float)pre[3]});
	return h4{(half_t)y[0], (half_t)y[1], (half_t)y[2], (half_t)y[3]};
}
TCNN_DEVICE_NOINLINE f4 act_derivative4_pre_general(uint32_t act, h4 pre) {
	f4 d;
	if (act == (uint32_t)Activation::Sine) {
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) d[j] = cosf((float)pre[j]);
	} else {  // SiLU
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const float x = (float)pre[j], l = 1.0f / (1.0f + expf(-x));
			d[j] = l + x * (l * (1.0f - l));
		}
	}
	return d;
}
// (T)((float)(T)v * (float)(T)f'(pre)).  NOT act_backward4's form, which multiplies the fp32 accumulator.
TCNN_DEVICE h4 act_backward4_pre(uint32_t act, f4 v, h4 pre) {
	mfma_settle(v);
	const f4 d = act_derivative4_pre_general(act, pre);
	h4 out;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) out[j] = (half_t)((float)(half_t)v[j] * (float)(half_t)d[j]);
	return out;
}

template <bool GENERAL>
TCNN_DEVICE float act_backward(uint32_t act, float v, half_t forward_value) {
	if (act == (uint32_t)Activation::ReLU) return forward_value > (half_t)0.0f ? v : 0.0f;
	if constexpr (GENERAL) {
		if (act != (uint32_t)Activation::None) return act_backward_general(act, v, forward_value);
	}
	return v;
}

// ---- activations on fp32 values, for the fp32 layer-by-layer network (mlp_general_fp32.hip; common_device.h:108-186 forward, :363-418 and
// :253-277 backward, with T = float): nothing is rounded.  ReLU / None stay inline as selects; everything else is ONE out-of-line body per
// kernel, entered once per fragment, like the 16-bit functions above that they mirror.
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

// ---- second derivatives, for the fp32 network's second-order pass (mlp_general_impl.h gen_backward_backward).  Through the same `aux` as
// the first: the post-activation value, or -- SiLU / Sine -- the pre-activation.  None, ReLU and LeakyReLU are piecewise linear: their second
// derivative is zero everywhere the first exists, and the pass skips every term that carries it.
TCNN_HOST_DEVICE bool act_second_derivative_is_zero(uint32_t act) {
	return act == (uint32_t)Activation::None || act == (uint32_t)Activation::ReLU || act == (uint32_t)Activation::LeakyReLU;
}
// v * f''(.)
TCNN_DEVICE_NOINLINE f4 act32_second4_general(uint32_t act, f4 v, f4 aux) {
	f4 out;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) {
		const float y = aux[j];
		float factor = 0.0f;
		switch ((Activation)act) {  // (uniform: hoisted out of the unrolled loop)
			case Activation::Exponential: factor = y; break;
			case Activation::Sigmoid: factor = y * (1.0f - y) * (1.0f - 2.0f * y); break;
			case Activation::Squareplus: {
				const float t = y * K_ACT, q = t * t + 1.0f;
				factor = (t * t / q) * (2.0f * t * K_ACT / (q * q));
				break;
			}
			case Activation::Softplus: {
				const float s = 1.0f - expf(-y * K_ACT);
				factor = K_ACT * s * (1.0f - s);
				break;
			}
			case Activation::Tanh: factor = -2.0f * y * (1.0f - y * y); break;
			case Activation::SiLU: {
				const float l = 1.0f / (1.0f + expf(-y));
				factor = l * (1.0f - l) * (2.0f + y * (1.0f - 2.0f * l));
				break;
			}
			case Activation::Sine: factor = -sinf(y); break;
			default: break;
		}
		out[j] = v[j] * factor;
	}
	return out;
}

}  // namespace tcnn_hip

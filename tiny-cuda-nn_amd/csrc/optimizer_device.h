// optimizer_device.h -- the per-parameter arithmetic of the optimizers besides Adam (adam_device.h), written once over the value type T
// of the weights / gradients / wrapper state: the library's 16-bit type (optimizer_kernels.hip, elementwise_kernels.hip) or float
// (optimizer_kernels_f32.hip -- the reference's Optimizer<float>, where every (T) cast is the identity).  Each function restates the
// reference's kernel operation by operation in the same fp32 order (build with -ffp-contract=off); reference lines are cited per function.
#pragma once
#include "tcnn_device.h"

namespace tcnn_hip {

// sgd.h:57-65
template <typename T>
TCNN_DEVICE float sgd_one(float loss_scale, float learning_rate, float l2_reg, float weight_fp, T gradient_raw) {
	float gradient = (float)gradient_raw / loss_scale;
	gradient += l2_reg * weight_fp;
	return weight_fp - learning_rate * gradient;
}

struct NovogradArgs {
	float relative_weight_decay, absolute_weight_decay, loss_scale, learning_rate, beta1, beta2, epsilon;
};
// novograd.h:62-69 with the layer's second moment in a register
template <typename T>
TCNN_DEVICE float novograd_one(const NovogradArgs& a, float second_moment, float weight_fp, T gradient_raw, float& first_moment) {
	const float gradient = (float)gradient_raw / a.loss_scale;
	first_moment = a.beta1 * first_moment + (1 - a.beta1) * gradient / (__builtin_sqrtf(second_moment) + a.epsilon);
	const float rel = a.relative_weight_decay * a.learning_rate, ab = a.absolute_weight_decay * a.learning_rate;
	const float decayed_weight = (1 - rel) * weight_fp - __builtin_copysignf(ab, weight_fp);  // common_device.h:1045-1048 weight_decay
	return decayed_weight - a.learning_rate * first_moment;
}
// novograd.h:84 from the layer's squared gradient norm
TCNN_DEVICE float novograd_second_moment(const NovogradArgs& a, float second_moment_in, float gradient_norm) {
	return a.beta2 * second_moment_in + (1 - a.beta2) * gradient_norm / a.loss_scale / a.loss_scale;
}

// lookahead.h:55
template <typename T>
TCNN_DEVICE float lookahead_one(float alpha, T slow, float weight_fp) { return (float)slow * (1.0f - alpha) + weight_fp * alpha; }

// average.h:56
template <typename T>
TCNN_DEVICE T average_one(float n_samples, T average, T weight, T sample) {
	return round_to<T>((float)average + ((float)weight - (float)sample) / n_samples);
}

// batched.h:60
template <typename T>
TCNN_DEVICE float batched_one(float pool, T gradient, float multiplier) { return pool + (float)gradient / multiplier; }

// ema.h:55-58
TCNN_DEVICE float ema_one(float old, float weight, float ema_decay, float ema_debias_old, float ema_debias_new) {
	return (old * ema_decay * ema_debias_old + weight * (1 - ema_decay)) * ema_debias_new;
}

}  // namespace tcnn_hip

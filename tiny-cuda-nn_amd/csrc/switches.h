// switches.h -- the process-wide A/B switches that the model passes and the trainer read.
#pragma once
#include <atomic>
#include <cstdint>

namespace tcnn_hip {

// Process-wide A/B switches (defined, and set through the C ABI, in api_switches.hip).
// grid backward formulation (GridBackwardMode); TCNN_GRID_BACKWARD=sliced_f32|sliced_f16|atomic|bucketed overrides the default
extern std::atomic<int> g_grid_backward_mode;
// Single-kernel network passes (process-wide; tcnn_set_fused_network_passes(0) turns them off):
//   * training_step: encoding forward, ONE kernel for the network's forward + loss + backward, encoding backward;
//   * forward() + backward() (Trainer and modules): the forward pass saves only the encoded input; the backward pass runs the same
//     kernel with the caller's dL/doutput in place of the loss -- it RECOMPUTES the hidden activations (three small matrix products)
//     instead of reading back what the forward pass would have had to write (2 B x width x layers per sample each way).
// Off: k_mlp_forward (saves the activations) -> k_loss -> k_mlp_backward.  Same results either way (tests/test_emu_kernels.py).
extern std::atomic<int> g_fused_network_passes;
// training_step: an unpadded Identity encoding is evaluated by the network kernel's own input loads (MlpF32Input) where an instance offers it;
// tcnn_set_fused_identity_input(0): always the separate encoding kernel (A/B runs, tests)
extern std::atomic<int> g_fused_identity_input;
// training_step(run_optimizer = 1) on one GPU sums the network kernel's weight-gradient slabs inside the optimizer's launch (AdamFinalize);
// tcnn_set_finalize_in_optimizer(0): always k_mlp_finalize_gradients, a launch of its own behind the network kernel (A/B runs, tests)
extern std::atomic<int> g_finalize_in_optimizer;
// second-order pass of an fp32 grid encoding: 0 = the fp32 kernels (default), 1 = the 16-bit kernels on stand-ins of the caller's fp32 tensors
// (tcnn_set_fp32_second_order; A/B runs, tests)
extern std::atomic<int> g_fp32_second_order;

}  // namespace tcnn_hip

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
// forward / inference of an fp32 network whose shape mlp_f32_fused_supported names: 1 = the fused kernel (mlp_f32_fused.hip, default), 0 = the
// layer-by-layer kernels at every shape (tcnn_set_fp32_fused_network; A/B runs, tests, the earlier bits)
extern std::atomic<int> g_fp32_fused_network;
// backward of an fp32 network whose shape mlp_f32_fused_backward_supported names: 1 = the fused chain and weight-gradient kernels
// (mlp_f32_fused_backward.hip, default), 0 = the layer-by-layer kernels (tcnn_set_fp32_fused_backward).  Read together with
// g_fp32_fused_network: that switch at 0 turns off every fused fp32 kernel, this one the backward pass alone.
extern std::atomic<int> g_fp32_fused_backward;
// second-order pass of the same networks: 1 = the fused tangent chain, reverse chain and dual weight-gradient kernels
// (mlp_f32_fused_second_order.hip, default), 0 = the layer-by-layer launches (tcnn_set_fp32_fused_second_order).  Read together with the
// two switches above: either of them at 0 turns the fused second-order pass off as well.
extern std::atomic<int> g_fp32_fused_second_order;
// parameter gradients of an fp32 grid encoding: 1 = the owner pass on the levels its plan takes (grid_backward_f32.hip, default), 0 = the
// reference's atomic kernel at every shape (tcnn_set_fp32_grid_backward; A/B runs, tests, the earlier bits)
extern std::atomic<int> g_fp32_grid_backward;
// forward of an fp32 grid encoding, with or without dy_dx: 1 = the level-major tiled gather on the forms it takes (grid_forward_f32.hip,
// default), 0 = the reference's one thread per (sample, level) at every form (tcnn_set_fp32_grid_forward; A/B runs, tests).  Same bits.
extern std::atomic<int> g_fp32_grid_forward;
// second-order pass of a lone fp32 grid encoding, a mask (tcnn_set_fp32_grid_second_order; grid_second_order_f32.hip): bit 0 = the parameter
// gradient through the owner pass (also needs g_fp32_grid_backward; default on), bit 1 = the level-major tiled input gradient (default off:
// slower where every table is L2-resident).  A cleared bit: the atomic
// scatter behind a memset of the table / one thread per sample walking the levels (A/B runs, tests, the earlier bits of dL_dparams).
extern std::atomic<int> g_fp32_grid_second_order;

}  // namespace tcnn_hip

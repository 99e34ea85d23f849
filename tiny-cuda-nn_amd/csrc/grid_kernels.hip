// grid_kernels.hip -- THE list of the grid encoding's translation units, one pass each.  csrc/Makefile reads its sources from the include
// lines below; the host emulator (tests/emu/emu_driver_grid.cpp) includes this file as its unity build.  Order: names before their use.
#if !defined(TCNN_HOST_EMU)
#error "grid_kernels.hip is a list, not a unit of the library: build grid_forward / grid_backward_scatter / grid_backward_owner / grid_backward / grid_second_order"
#endif
#include "grid_forward.hip"
#include "grid_backward_scatter.hip"
#include "grid_backward_owner.hip"
#include "grid_backward.hip"
#include "grid_second_order.hip"

// The fp32 launchers were spelled with a suffix before they became overloads on float.  A host emulator driver of that spelling -- the
// suite of the revision before is expected to build against these sources -- finds the four names here.  Nothing in the library does: this
// file is not one of its units.
namespace tcnn_hip {
inline void grid_forward_f32(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* params, float* out, float* dy_dx = nullptr) { grid_forward(stream, meta, io, params, out, dy_dx); }
inline void grid_backward_f32(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* dL_dy, float* grid_gradient, bool accumulate) {
	grid_backward(stream, meta, io, dL_dy, grid_gradient, accumulate);
}
inline void grid_backward_input_f32(hipStream_t stream, uint32_t n_dims, uint32_t n_features, const GridIO& io, const float* dL_dy, const float* dy_dx, float* dL_dx, uint32_t dx_stride_i,
                                    uint32_t dx_stride_d) {
	grid_backward_input(stream, n_dims, n_features, io, dL_dy, dy_dx, dL_dx, dx_stride_i, dx_stride_d);
}
inline void grid_backward_backward_input_f32(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* dL_dy, const float* params, float* dL_dx, uint32_t dx_stride_i,
                                             uint32_t dx_stride_d) {
	grid_backward_backward_input(stream, meta, io, dL_dy, params, dL_dx, dx_stride_i, dx_stride_d);
}
}  // namespace tcnn_hip

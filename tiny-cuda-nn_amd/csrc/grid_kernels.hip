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

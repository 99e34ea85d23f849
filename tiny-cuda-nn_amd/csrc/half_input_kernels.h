// half_input_kernels.h -- a bare network fed the caller's own 16-bit matrix (tcnn_module_*_half_input): the two streaming kernels between
// the caller's sample-major [n][n_dims] matrices and the feature-major [padded][n] matrices the network kernels read and write
// (mlp_kernels.h "Data layout at the kernel boundary").  They stand where the Identity encoding (scale 1, offset 0) and its backward pass
// stand on the fp32 route, and leave the same bits: the identity is exact on values the 16-bit type holds, so nothing is computed here --
// 16-bit words are moved, whichever of the two 16-bit types the build has.
#pragma once
#include "tcnn_device.h"

namespace tcnn_hip {

// out[k][i] = in[i][k] for k < n_dims, the 16-bit pattern `pad_bits` for n_dims <= k < padded (identity.h:62-64 pads with 1)
void half_input_pad(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t padded, const uint16_t* in, uint16_t* out, uint16_t pad_bits);
// dL_dx[i][k] = dL_dy[k][i] for k < n_dims; rows n_dims .. of dL_dy (the padding's gradient) are not read
void half_input_unpad(hipStream_t stream, uint32_t n, uint32_t n_dims, const uint16_t* dL_dy, uint16_t* dL_dx);

}  // namespace tcnn_hip

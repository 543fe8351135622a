// trtlab_amd — conv2d implicit-GEMM kernels, int8_t instantiation.
#include "conv_igemm.h"

namespace trtlab {

template void launch_conv2d_t<int8_t>(
    const void* in, const void* Wt, void* out, const float* scale,
    const float* bias, const void* residual, const void* zero_page,
    const ConvParams& p, int epi, hipStream_t stream, int tile,
    float* scratch, int staging);

}  // namespace trtlab

// trtlab_amd — conv2d implicit-GEMM kernels, __bf16 instantiation.
#include "conv_igemm.h"

namespace trtlab {

template void launch_conv2d_t<__bf16>(
    const void* in, const void* Wt, void* out, const float* scale,
    const float* bias, const void* residual, const void* zero_page,
    const ConvParams& p, int epi, hipStream_t stream, int tile,
    float* scratch, int staging);

}  // namespace trtlab

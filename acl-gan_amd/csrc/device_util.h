// device_util.h -- the device helpers more than one translation unit needs: the activation and its derivative, the wavefront sum and the
// two sums over a 256-thread workgroup.  One definition each; every kernel that applies an activation or reduces over a workgroup uses these.
#pragma once
#include "common.h"

namespace aclgan {

__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == ACLGAN_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == ACLGAN_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
    if (act == ACLGAN_ACT_TANH) return tanhf(v);
    return v;
}
// derivative of the activation expressed through its OUTPUT y
__device__ __forceinline__ float act_grad(float y, int act) {
    if (act == ACLGAN_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    if (act == ACLGAN_ACT_LRELU) return y > 0.f ? 1.f : 0.2f;
    if (act == ACLGAN_ACT_TANH) return 1.f - y * y;
    return 1.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The two workgroup sums differ in where the barriers stand and in who holds the result: they are not interchangeable.
// block-wide sum for 256-thread blocks; result valid in every thread
__device__ __forceinline__ float block_sum256(float v, float* red /*[4]*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
// sum over a 256-thread block, valid in thread 0
__device__ __forceinline__ float block_sum_t0(float v) {
    __shared__ float red[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return r;
}

}  // namespace aclgan

// What the gathers behind an align-corners zoom share (seg_loss.hip, msc.hip): the source cell of an output coordinate, the range of
// output coordinates that touch a cell, and the workgroup's sum in a fixed order.  One copy: both files' bit-for-bit contracts rest on
// the same footprints and the same tree.
#pragma once
#include <hip/hip_runtime.h>

namespace dsrg {

// the source cell of output coordinate d on an axis of n_in samples (eval.hip: the min never binds)
__device__ __forceinline__ int sl_cell(double scale, int d, int n_in) { return min((int)(scale * (double)d), n_in - 1); }

// the first output coordinate in [0, n_out] whose source cell is >= i (source cells never decrease along the axis)
__device__ inline int sl_first(double scale, int i, int n_in, int n_out) {
    if (i <= 0) return 0;
    if (i > n_in - 1 || !(scale > 0.0)) return n_out;
    const double q = ceil((double)i / scale);
    int g = q < (double)n_out ? (int)q : n_out;
    while (g > 0 && sl_cell(scale, g - 1, n_in) >= i) --g;
    while (g < n_out && sl_cell(scale, g, n_in) < i) ++g;
    return g;
}

// the sum of v over a workgroup of N lanes in a fixed order (a tree over the lane index); every lane gets it
template <int N, typename T>
__device__ __forceinline__ T sl_block_sum(T v, T *s_red) {
    const int tid = threadIdx.x;
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int k = N / 2; k > 0; k >>= 1) {
        if (tid < k) s_red[tid] = s_red[tid] + s_red[tid + k];
        __syncthreads();
    }
    return s_red[0];
}

}  // namespace dsrg

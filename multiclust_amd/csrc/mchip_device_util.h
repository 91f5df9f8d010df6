/*
 * mchip_device_util.h -- the building blocks every device unit shares: LDS row staging at an odd pitch, the fixed summation tree
 * over a workgroup's lanes, sums of partials in one fixed order, integer counts through atomics.  Rule of the library: no floating-point atomics, one fixed order per
 * sum, so that the same state gives the same bits; a new unit's kernel is its body plus calls of these.
 */
#ifndef MCHIP_DEVICE_UTIL_H
#define MCHIP_DEVICE_UTIL_H

#include <hip/hip_runtime.h>

#define MCHIP_BLOCK 256	/* lanes per workgroup of the library's own kernels */

/* doubles between two LDS rows of K doubles that the lanes of a wave read side by side (lane i its own row: q rows, staged P rows).
 * Lane i reads dwords 2 (pitch i + k) and the next one; with the pitch odd the 32 lanes of a ds_read_b64 lane group fall on 32
 * different bank pairs of the 64. */
__host__ __device__ constexpr int lds_pitch(int K) { return K | 1; }

/* nrows rows of K contiguous doubles from src into LDS rows `pitch` apart: consecutive threads read consecutive doubles.  Every
 * thread of the workgroup calls it (tid of nthr); the caller's barrier follows. */
__device__ __forceinline__ void stage_rows(double *dst, int pitch, const double *__restrict__ src, int nrows, int K, int tid, int nthr)
{
	for (int x = tid; x < nrows * K; x += nthr) dst[(x / K) * pitch + x % K] = src[x];
}

/* the q rows of the workgroup's individuals i0 .. i0 + nthr - 1 (those below I), lane order = row order; Q is a slot's [I][K]
 * (qstride = K) or the shared [K] (qstride = 0), which every row then holds */
__device__ __forceinline__ void stage_q_rows(double *qs, int pitch, const double *__restrict__ Q, int qstride, int i0, int I, int K, int tid,
					      int nthr)
{
	if (qstride) {
		stage_rows(qs, pitch, Q + (size_t)i0 * K, max(0, min(nthr, I - i0)), K, tid, nthr);
	} else {
		for (int x = tid; x < nthr * K; x += nthr) qs[(x / K) * pitch + x % K] = Q[x % K];
	}
}

/* The fixed tree over the lanes of a workgroup -- NT of them, or blockDim.x with NT = 0; a power of two -- for NV values at a time
 * in red[NV][pitch]: lane t stores its values, then red[.][t] += red[.][t + w] for w = lanes / 2 ... 1, one barrier per level however
 * many values travel.  Every thread calls it; the sums are in red[.][0] for every thread after the last barrier, which is not
 * followed by another: a caller that writes red[] again puts one in between. */
template <int NT = 0, int NV, typename T> __device__ __forceinline__ void block_tree_sum(T *red, int pitch, const T (&v)[NV])
{
	static_assert(NV >= 1 && NV <= 3, "one, two or three values");
	const int tid = threadIdx.x;
	red[tid] = v[0];
	if constexpr (NV > 1) red[pitch + tid] = v[1];
	if constexpr (NV > 2) red[2 * pitch + tid] = v[2];
	__syncthreads();
	for (int w = (NT ? NT : (int)blockDim.x) >> 1; w > 0; w >>= 1) {
		if (tid < w) {
			red[tid] += red[tid + w];
			if constexpr (NV > 1) red[pitch + tid] += red[pitch + tid + w];
			if constexpr (NV > 2) red[2 * pitch + tid] += red[2 * pitch + tid + w];
		}
		__syncthreads();
	}
}
/* one value: the sum itself */
template <int NT = 0, typename T> __device__ __forceinline__ T block_tree_sum(T *red, T v)
{
	const T one[1] = {v};
	block_tree_sum<NT>(red, 0, one);
	return red[0];
}

/* global[x] += the workgroup's sum of mine[x], x < N: integers, the order does not matter.  One LDS atomic per lane and non-zero
 * count, then one global atomic per workgroup and non-zero count.  Every thread calls it. */
template <int N> __device__ __forceinline__ void block_add_counts(const unsigned long long (&mine)[N], unsigned long long *global)
{
	__shared__ unsigned long long cnt[N];
	if (threadIdx.x == 0)
		for (int x = 0; x < N; x++) cnt[x] = 0;
	__syncthreads();
	for (int x = 0; x < N; x++)
		if (mine[x]) atomicAdd(&cnt[x], mine[x]);
	__syncthreads();
	if (threadIdx.x == 0)
		for (int x = 0; x < N; x++)
			if (cnt[x]) atomicAdd(&global[x], cnt[x]);
}

/* acc + in[first] + in[first + stride] + ... (count terms, added in that order): the loads of eight terms are issued
 * together, the additions keep their order, so the result is the plain loop's to the last bit */
__device__ __forceinline__ double ordered_sum(double acc, const double *__restrict__ in, size_t first, size_t stride, int count)
{
	int x = 0;
	for (; x + 8 <= count; x += 8) {
		double v[8];
#pragma unroll
		for (int y = 0; y < 8; y++) v[y] = in[first + (size_t)(x + y) * stride];
#pragma unroll
		for (int y = 0; y < 8; y++) acc += v[y];
	}
	for (; x < count; x++) acc += in[first + (size_t)x * stride];
	return acc;
}

/* deterministic sum of n doubles by one block (fixed strided order, then a fixed tree); every thread must call it; the result is
 * valid in thread 0 (and red[] may be reused after the trailing barrier) */
__device__ __forceinline__ double block_ordered_sum(const double *__restrict__ in, int n, double *red)
{
	const double s = (int)threadIdx.x < n ? ordered_sum(0.0, in, threadIdx.x, MCHIP_BLOCK, (n - (int)threadIdx.x + MCHIP_BLOCK - 1) / MCHIP_BLOCK) : 0.0;
	const double v = block_tree_sum<MCHIP_BLOCK>(red, s);
	__syncthreads();
	return v;
}

#endif

/*
 * mchip_resample.hip -- a data set made of a selection of loci with repeats: the kernel behind mchip_resample_loci
 * (include/multiclust_hip.h has the contract; mchip.hip has the entry point and the per-context state).
 *
 *   k_resample_gather   out[i][j][.] = base[i][src[j]][.], both in upload form.  A workgroup takes a chunk of RS_CHUNK output
 *                       loci and stages their source indices in LDS once; it then walks individuals (blockIdx.y, grid stride).
 *                       Within an individual consecutive threads take consecutive output loci, so a wave writes 64 * ploidy
 *                       contiguous bytes of one individual's output row and its reads stay inside that individual's base row
 *                       (L_base * ploidy bytes: 200 KB at the headline shape, which the L2 cache holds while the chunks of the
 *                       row are gathered).  Every index is 64-bit: I * L * ploidy is 2 * 10^9 at the headline shape.
 *                       A thread that met an observed copy marks its individual, as k_cv_mask does.
 *                       Measured cost: profiles/locus_bootstrap.txt.
 */
#include "mchip_internal.h"

constexpr int RS_CHUNK = 1024;	/* output loci per workgroup: 4 KB of staged indices, four loci per thread and individual */

__global__ __launch_bounds__(256) void k_resample_gather(const uint8_t *__restrict__ base, const int32_t *__restrict__ src, int I,
							 int L_base, int L2, int pl, uint8_t *__restrict__ out, uint8_t *seen)
{
	__shared__ int32_t s_src[RS_CHUNK];
	const int j0 = blockIdx.x * RS_CHUNK, nj = min(RS_CHUNK, L2 - j0);
	for (int x = threadIdx.x; x < nj; x += 256) s_src[x] = src[j0 + x];
	__syncthreads();
	for (int i = blockIdx.y; i < I; i += gridDim.y) {
		const uint8_t *__restrict__ brow = base + (size_t)i * L_base * pl;
		uint8_t *__restrict__ orow = out + ((size_t)i * L2 + j0) * pl;
		bool any = false;
		for (int x = threadIdx.x; x < nj; x += 256) {
			const uint8_t *g = brow + (size_t)s_src[x] * pl;
			for (int a = 0; a < pl; a++) {
				const uint8_t v = g[a];
				any |= v != MCHIP_MISSING;
				orow[(size_t)x * pl + a] = v;
			}
		}
		if (any) seen[i] = 1;	/* (every writer stores the same value) */
	}
}

void mchip_resample_gather(hipStream_t s, const uint8_t *base, const int32_t *src, int I, int L_base, int L2, int ploidy, uint8_t *out,
			   uint8_t *seen)
{
	const unsigned chunks = (unsigned)((L2 + RS_CHUNK - 1) / RS_CHUNK);
	/* enough workgroups to fill the device many times over, each staging its indices for several individuals */
	unsigned rows = (unsigned)I;
	const unsigned want = (65536u + chunks - 1) / chunks;
	if (rows > want) rows = want;
	if (rows > 65535u) rows = 65535u;
	hipLaunchKernelGGL(k_resample_gather, dim3(chunks, rows), dim3(256), 0, s, base, src, I, L_base, L2, ploidy, out, seen);
}

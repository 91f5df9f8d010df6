/* lane_pass_geometry_of (multiclust_amd/csrc/mchip_feature_geometry.h) as a program of its own, for tests/test_feature_geometry_cpu.py:
 * feature_geometry_driver I L n_cu red_bytes min_threads lds_budget  ->  one line per K = 1 .. 64 and max_M = 1 .. 255:
 * K max_M threads stage lds n_itiles lchunk n_lchunks */
#include "mchip_feature_geometry.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
	if (argc != 7) return 2;
	const int I = atoi(argv[1]), L = atoi(argv[2]), n_cu = atoi(argv[3]), min_threads = atoi(argv[5]);
	const size_t red = (size_t)atol(argv[4]), budget = (size_t)atol(argv[6]);
	for (int K = 1; K <= 64; K++)
		for (int max_M = 1; max_M <= 255; max_M++) {
			const lane_pass_geometry g = lane_pass_geometry_of(I, L, K, max_M, n_cu, red, min_threads, budget);
			printf("%d %d %d %d %zu %d %d %d\n", K, max_M, g.threads, g.stage, g.lds, g.n_itiles, g.lchunk, g.n_lchunks);
		}
	return 0;
}

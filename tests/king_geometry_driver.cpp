/* king_geometry_of (multiclust_amd/csrc/mchip_feature_geometry.h) as a program of its own, for tests/test_king_cpu.py:
 * king_geometry_driver  <  lines "I n_rows L target_blocks"  ->  one line each:
 * KING_TILE KING_STAGE n_rtiles n_ctiles n_split stages_per_split */
#include "mchip_feature_geometry.h"

#include <stdio.h>

int main()
{
	int I, n_rows, L;
	long long target;
	while (scanf("%d %d %d %lld", &I, &n_rows, &L, &target) == 4) {
		const king_geometry g = king_geometry_of(I, n_rows, L, target);
		printf("%d %d %d %d %d %d\n", KING_TILE, KING_STAGE, g.n_rtiles, g.n_ctiles, g.n_split, g.stages_per_split);
	}
	return 0;
}

/* qc_geometry_of (multiclust_amd/csrc/mchip_feature_geometry.h) as a program of its own, for tests/test_qc_cpu.py:
 * qc_geometry_driver  <  lines "I L target_blocks"  ->  one line each:
 * QC_VARIANTS QC_STEP QC_ITILE n_vgroups v_split steps_per_split n_itiles i_split words_per_split */
#include "mchip_feature_geometry.h"

#include <stdio.h>

int main()
{
	int I, L;
	long long target;
	while (scanf("%d %d %lld", &I, &L, &target) == 3) {
		const qc_geometry g = qc_geometry_of(I, L, target);
		printf("%d %d %d %d %d %d %d %d %d\n", QC_VARIANTS, QC_STEP, QC_ITILE, g.n_vgroups, g.v_split, g.steps_per_split, g.n_itiles, g.i_split,
		       g.words_per_split);
	}
	return 0;
}

/* The RANSAC PnP entry points of include/betapose_hip.h seen from plain C (gcc -std=c99 -pedantic -Wall -Werror): the
 * prototypes compile and have the documented types, and the host-only ones answer.  Needs no GPU.
 *   gcc -std=c99 -pedantic -Wall -Werror -Iinclude examples/pnp_ransac_abi_check.c -o /tmp/pnp_ransac_abi_check \
 *       -Lbetapose_amd -lbetapose_hip -Wl,-rpath,$PWD/betapose_amd */
#include <stdio.h>
#include "betapose_hip.h"
int main(void) {
    int idx[5 * 6], need[11], i, j;
    int (*batch)(const double*, int, const double*, int, int, const double*, double, int, double, double*, int*, unsigned char*,
                 void*, size_t, void*) = bp_solve_pnp_ransac_batch;
    int (*set)(bp_pipeline*, double, int, double) = bp_pipeline_set_pose_ransac;
    int (*rec)(const float*, int, const double*, int, const double*, int, double, int, double, double*, void*, size_t,
               void*) = bp_pose_from_records_ransac;
    if (!batch || !set || !rec) return 1;
    if (bp_pnp_ransac_samples(10, 5, idx) != 0) return 2;
    for (i = 0; i < 5; ++i)
        for (j = 0; j < 6; ++j)
            if (idx[i * 6 + j] < 0 || idx[i * 6 + j] >= 10) return 3;
    if (bp_pnp_ransac_trials_needed(10, 0.99, need) != 0 || need[10] != 1) return 4;
    if (bp_pnp_ransac_samples(5, 5, idx) == 0) return 5;                 /* fewer than six points: refused */
    if (bp_pnp_ransac_workspace_bytes(28, 100) < (size_t)28 * 100 * 12) return 6;
    if (bp_pose_ransac_workspace_bytes(28, 100) <= bp_pnp_ransac_workspace_bytes(28, 100)) return 7;
    if (set(NULL, 12.0, 100, 0.99) == 0) return 8;                       /* no pipeline: an error, not a crash */
    printf("idx0 %d need[5] %d\n", idx[0], need[5]);
    return 0;
}

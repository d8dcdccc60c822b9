// Prints the plans of genpc_amd/csrc/pose_plan.h for shapes given on the command line, as genpc_pose_loss_grad_batch asks for them
// (b scans, one start, no side stream, the switches at their defaults).  Host code only; tests/test_pose_step_shapes.py builds it
// with -fsanitize=address,undefined, runs it on the rows of tests/pose_step_shapes.py and asserts what each row must select.
// Arguments: groups of six -- b nc np radius S mask(0/1).  One line per group:
//   b nc np elements ride g_t g_g gb sub8 fuse_w gp gs lin_nc lin_nc_np lin_8nc
// (sub8 ... gs are -1 without the mask term: there is no silhouette step to plan.)
#include "pose_plan.h"

#include <stdio.h>
#include <stdlib.h>

using namespace genpc;

int main(int argc, char **argv)
{
    if (argc < 7 || (argc - 1) % 6 != 0) {
        fprintf(stderr, "usage: %s (b nc np radius S mask)...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 5 < argc; i += 6) {
        const int b = atoi(argv[i]), nc = atoi(argv[i + 1]), np = atoi(argv[i + 2]), S = atoi(argv[i + 4]), mask = atoi(argv[i + 5]);
        const float radius = (float)atof(argv[i + 3]);
        if (b <= 0 || nc <= 0 || np <= 0 || (mask && (S <= 1 || !(radius > 0.0f)))) {
            fprintf(stderr, "bad shape in group %d\n", (i - 1) / 6);
            return 2;
        }
        PoseLoopAsk a;
        a.scans = b; a.starts = 1; a.nc = nc; a.np = np; a.mask = mask != 0;
        a.side_stream_ok = false;
        a.counters_ok = false;
        const PoseLoopPlan p = pose_loop_plan(a);
        MaskStepPlan m{};
        if (mask) m = mask_step_plan(p.elements, nc, S, radius);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", b, nc, np, p.elements, (int)p.ride, p.g_t, p.g_g, p.gb, mask ? (int)m.sub8 : -1,
               mask ? (int)m.fuse_w : -1, mask ? m.gp : -1, mask ? m.gs : -1, lin_grid(nc), lin_grid((long long)nc + np), lin_grid(8ll * nc));
    }
    return 0;
}

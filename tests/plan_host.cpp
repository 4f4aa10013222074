// Stand-alone driver of fwi::plan_context (csrc/fwi_plan.h) on the CPU.  Built from csrc/fwi_plan.cpp with
// -fsanitize=address,undefined and run by tests/test_plan_host.py; the hooks reach it through its environment.
//   plan_host plan       one configuration per line of stdin, as fifteen integers, the members of fwi_config from ndim to
//                        store_dtype without `device` (ndim nz ny nx order nt_max npml dtype kernel zchunk
//                        ckpt_interval image_stride update_form abc store_dtype); one line of tab-separated fields out:
//                        code, reason, report line, kernel name, place_kind, place_mode, fixed_k, inc, tuning
//                        (ty zchunk pf tile_x), ptot, esize
//   plan_host threshold  the size threshold of the placement search on both sides, from make_grid alone; exit status 0 =
//                        every check held
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "fwi_plan.h"

using namespace fwi;

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

fwi_config config(int ndim, int nz, int ny, int nx) {
    fwi_config c{};
    c.struct_size = (int32_t)sizeof(fwi_config);
    c.ndim = ndim;
    c.nz = nz;
    c.ny = ny;
    c.nx = nx;
    c.order = 8;
    c.nt_max = 8;
    c.dtype = FWI_F32;
    c.h = 10.0;
    c.dt = 1e-3;
    c.sigma_max = 900.0;
    return c;
}

int run_plans() {
    const Hooks hooks = Hooks::from_env();
    char row[512];
    while (fgets(row, sizeof row, stdin)) {
        int v[15];
        if (sscanf(row, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8,
                   v + 9, v + 10, v + 11, v + 12, v + 13, v + 14) != 15) {
            fprintf(stderr, "plan_host: malformed line: %s", row);
            return 2;
        }
        fwi_config c = config(v[0], v[1], v[2], v[3]);
        c.order = v[4];
        c.nt_max = v[5];
        c.npml = v[6];
        c.dtype = v[7];
        c.kernel = v[8];
        c.zchunk = v[9];
        c.ckpt_interval = v[10];
        c.image_stride = v[11];
        c.update_form = v[12];
        c.abc = v[13];
        c.store_dtype = v[14];
        Plan p;
        std::string why;
        const int rc = plan_context(c, hooks, &p, &why);
        char line[160] = "";
        // (what fwi_create does: the line of a plan that was decided, also where "fixed:" is then refused)
        if (rc == FWI_OK || p.place_kind) plan_report(p, line, sizeof line);
        printf("%d\t%s\t%s\t%s\t%d\t%d\t", rc, why.c_str(), line, rc == FWI_OK ? plan_kernel_name(p) : "", p.place_kind,
               (int)p.place_mode);
        for (int i = 0; i < 8; ++i) printf("%s%d", i ? "," : "", p.fixed_k[i]);
        printf("\t%d\t%d %d %d %d\t%lld\t%zu\n", (int)p.inc, p.tune.ty, p.tune.zchunk, p.tune.pf, p.tune.tile_x,
               (long long)p.gd.ptot, p.esize);
    }
    return 0;
}

// The search is on from ptot * esize >= 48e6 (3-D fp32 stream contexts that place): the first nz at which a 200 x 200
// plane reaches it, found from make_grid alone, and the one below it.
int run_threshold() {
    const Hooks hooks;  // no hook set
    int nz = 1;
    while ((double)make_grid(3, nz, 200, 200, 8).ptot * 4 < 48e6) ++nz;
    CHECK(nz > 16 && nz < 2000);
    CHECK((double)make_grid(3, nz - 1, 200, 200, 8).ptot * 4 < 48e6);
    for (int cpml = 0; cpml < 2; ++cpml) {
        for (int below = 0; below < 2; ++below) {
            fwi_config c = config(3, nz - below, 200, 200);
            c.npml = 8;
            c.abc = cpml ? FWI_ABC_CPML : FWI_ABC_SPONGE;
            c.update_form = cpml ? FWI_UPDATE_STANDARD : FWI_UPDATE_INCREMENT;
            Plan p;
            std::string why;
            CHECK(plan_context(c, hooks, &p, &why) == FWI_OK);
            CHECK(p.kernel == K_STREAM && p.xpml == (cpml != 0));
            CHECK(p.place_kind == (below ? 0 : cpml ? 1 : 2));
            CHECK(p.place_mode == (below ? PLACE_OFF : PLACE_SEARCH));
            CHECK(p.place_pad == (below ? 0 : (size_t)14 << 20));
            // fp64 and the point kernel never place, whatever the size
            c.dtype = FWI_F64;
            CHECK(plan_context(c, hooks, &p, &why) == FWI_OK && p.place_kind == 0 && p.place_mode == PLACE_OFF);
            c.dtype = FWI_F32;
            c.kernel = FWI_KERNEL_POINT;
            CHECK(plan_context(c, hooks, &p, &why) == FWI_OK && p.place_kind == 0 && p.place_mode == PLACE_OFF);
        }
    }
    printf("threshold: nz = %d at 200 x 200 (ptot %lld)\n", nz, (long long)make_grid(3, nz, 200, 200, 8).ptot);
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return run_plans();
    if (argc == 2 && !strcmp(argv[1], "threshold")) return run_threshold();
    fprintf(stderr, "usage: plan_host plan < configurations | plan_host threshold\n");
    return 2;
}

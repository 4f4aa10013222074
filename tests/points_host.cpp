// Stand-alone driver of a shot's point tables (csrc/fwi_points.h) on the CPU.  Built from csrc/fwi_plan.cpp and
// csrc/fwi_points.cpp with -fsanitize=address,undefined and run by tests/test_points_host.py; the hooks reach it through
// its environment.  Input is blank-separated integers on stdin, output one "name v v v ..." line per array.
//   points_host tables   per case: the fifteen integers of plan_host's input line (fwi_config from ndim to store_dtype
//                        without `device`), n, then the n x ndim grid indices.  Out: "rc", and for a plan that was decided
//                        "plan" (kernel ty zchunk tile_x fused2d fused_ft cpml pair3d pair_zc pair_tw r cx sy sz off0),
//                        "outside" (flatten's answer) and, where that is -1, every table the plan calls for; "end".
//   points_host spread   per case: npts nnodes, whether pt_start and the weights are given (0 / 1), the length of
//                        pt_start and its entries.  Out: "spread" check point count, then the owners.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fwi_plan.h"
#include "fwi_points.h"

using namespace fwi;

namespace {

bool read_int(int *v) { return scanf("%d", v) == 1; }

template <typename V>
void row(const char *name, const std::vector<V> &v) {
    printf("%s", name);
    for (const V &x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int run_tables() {
    const Hooks hooks = Hooks::from_env();
    int v[15];
    while (read_int(v)) {
        int n;
        for (int i = 1; i < 15; ++i)
            if (!read_int(v + i)) return 2;
        if (!read_int(&n) || n < 0) return 2;
        fwi_config c{};
        c.struct_size = (int32_t)sizeof(fwi_config);
        c.ndim = v[0], c.nz = v[1], c.ny = v[2], c.nx = v[3], c.order = v[4], c.nt_max = v[5], c.npml = v[6];
        c.dtype = v[7], c.kernel = v[8], c.zchunk = v[9], c.ckpt_interval = v[10], c.image_stride = v[11];
        c.update_form = v[12], c.abc = v[13], c.store_dtype = v[14];
        c.h = 10.0, c.dt = 1e-3, c.sigma_max = 900.0;
        std::vector<int32_t> idx((size_t)n * c.ndim);  // (exactly as long as the tables may read)
        for (int32_t &x : idx)
            if (!read_int(&x)) return 2;
        Plan p;
        std::string why;
        const int rc = plan_context(c, hooks, &p, &why);
        printf("rc %d\n", rc);
        if (rc == FWI_OK) {
            const GridDesc &g = p.gd;
            printf("plan %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld\n", p.kernel, p.tune.ty, p.tune.zchunk,
                   p.tune.tile_x, (int)p.fused2d, p.fused_ft, (int)p.cpml, (int)p.pair3d, p.pair_zc, p.pair_tw, g.r, g.cx,
                   (long long)g.sy, (long long)g.sz, (long long)g.off0);
            FlatPoints flat;
            const int outside = flatten(g, idx.data(), n, &flat);
            printf("outside %d\n", outside);
            if (outside < 0) {
                row("pidx", flat.pidx);
                row("cidx", flat.cidx);
                StepTable st;
                step_table(p, idx.data(), n, flat, &st);
                row("step.start", st.start), row("step.pidx", st.pidx), row("step.cidx", st.cidx);
                row("step.col", st.col), row("step.run", st.run);
                if (p.fused2d) {
                    Fused2dTables ft;
                    fused2d_tables(p, idx.data(), n, &ft);
                    row("fused.start", ft.start), row("fused.lz", ft.lz), row("fused.lx", ft.lx), row("fused.col", ft.col);
                    row("fused.interior", ft.interior), row("fused.run", ft.run);
                    row("fused.rstart", ft.rstart), row("fused.rlz", ft.rlz), row("fused.rlx", ft.rlx);
                    row("fused.rcol", ft.rcol);
                }
                if (p.pair3d) {
                    Pair3dTable pt;
                    pair3d_table(p, idx.data(), n, &pt);
                    row("pair.start", pt.start);
                    std::vector<int> e;
                    for (const Pair3dInj &q : pt.ent) {
                        if (q.cu != 0.f) return 3;  // (the caller's to fill)
                        e.insert(e.end(), {q.z, q.yoff, q.xoff, q.col, q.interior});
                    }
                    row("pair.ent", e);
                }
            }
        }
        printf("end\n");
    }
    return 0;
}

int run_spread() {
    int npts, nnodes, have_start, have_weight, len;
    while (read_int(&npts)) {
        if (!read_int(&nnodes) || !read_int(&have_start) || !read_int(&have_weight) || !read_int(&len) || len < 0) return 2;
        std::vector<int32_t> start((size_t)len);
        for (int32_t &x : start)
            if (!read_int(&x)) return 2;
        const SpreadOwners so = spread_owners(npts, nnodes, have_start ? start.data() : nullptr, have_weight != 0);
        printf("spread %d %d %d", (int)so.check, so.point, so.count);
        for (int o : so.owner) printf(" %d", o);
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    static_assert(sizeof(Pair3dInj) == 24, "the two-step kernel reads six 4-byte fields per entry");
    if (argc == 2 && !strcmp(argv[1], "tables")) return run_tables();
    if (argc == 2 && !strcmp(argv[1], "spread")) return run_spread();
    fprintf(stderr, "usage: points_host tables < cases | points_host spread < cases\n");
    return 2;
}

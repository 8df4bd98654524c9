/* Prints what the search planner (sptag_amd/csrc/plan.h) decides for a fixed
 * list of cases, one line each; tests/test_search_plan.py compiles this with
 * the host compiler and compares the lines with values worked by hand. */
#include <cstdio>

#include "plan.h"

using namespace sptag_amd;

static IndexParams index_of(int algo, int dim, size_t esz)
{
    return {algo, dim, esz, INIT_PIVOTS, OTHER_PIVOTS, 3};
}

static SearchKnobs knobs(int ng_cap, int glevels, bool prof)
{
    SearchKnobs k;
    k.ng_cap_override = ng_cap;
    k.ng_glevels = glevels;
    k.prof = prof;
    return k;
}

static void show(const char* name, const IndexParams& ix, int32_t k, int32_t mc,
                 bool refine, int lds_limit, const SearchKnobs& kn, bool detail = false)
{
    const SearchPlan p = plan_search(ix, k, mc, refine, lds_limit, kn);
    const SearchCfg& c = p.lds;
    printf("%s: nq=%d k=%d mc=%d piv=%d/%d/%d dup=%d del=%d dpq=%d vcap=%d ng=%d "
           "spt=%d lsplit=%d global=%d/%d lds=%zu lds_ok=%d ng_tail=%d prof=%d "
           "sstride=%d\n",
           name, c.nq, c.k, c.max_check, c.init_pivots, c.other_pivots,
           c.nobetter_threshold, c.search_dup, c.search_deleted, c.dpq_cap, c.vcap,
           c.ng_cap, c.spt_cap, c.ng_lsplit, p.g_ng_cap, p.g_spt_cap, p.lds_total,
           (int)p.lds_ok, (int)p.ng_tail, c.prof, p.sstride);
    if (!detail) return;
    printf("%s scratch: visited=%zu gspt0=%zu gng0=%zu gng=%zu gspt=%zu\n", name,
           p.visited_bytes, p.gspt0_bytes, p.gng0_bytes, p.gng_bytes, p.gspt_bytes);
}

int main()
{
    const IndexParams bkt = index_of(ALGO_BKT, 128, 4);
    const IndexParams kdt = index_of(ALGO_KDT, 128, 4);
    const int LDS64K = 65536, LDS160K = 163840;

    show("bkt_mc2048", bkt, 10, 2048, false, LDS64K, SearchKnobs{}, true);
    show("bkt_refine", bkt, 501, 8192, true, LDS64K, SearchKnobs{}, true);
    show("bkt_mc16", bkt, 10, 16, false, LDS64K, SearchKnobs{});
    show("kdt_mc512", kdt, 10, 512, false, LDS64K, SearchKnobs{});
    show("cap384_g2", bkt, 10, 2048, false, LDS64K, knobs(384, 2, false));
    show("cap100", bkt, 10, 2048, false, LDS64K, knobs(100, NG_GLEVELS, false));
    show("i8_d100", index_of(ALGO_BKT, 100, 1), 10, 2048, false, LDS64K, SearchKnobs{});
    /* glevels outside 0..3 are clamped */
    show("g9", bkt, 10, 2048, false, LDS64K, knobs(0, 9, false));
    show("g_neg", bkt, 10, 2048, false, LDS64K, knobs(0, -1, false));
    /* the 64 KiB bound holds whatever the device reports; a smaller device
     * limit holds too */
    show("d4096_g0", index_of(ALGO_BKT, 4096, 4), 1024, 8192, false, LDS160K,
         knobs(0, 0, false), true);
    show("d4096_g3", index_of(ALGO_BKT, 4096, 4), 1024, 8192, false, LDS160K,
         knobs(0, 3, false));
    show("small_device", bkt, 10, 2048, false, 4096, SearchKnobs{});
    show("bkt_prof", bkt, 10, 2048, false, LDS64K, knobs(0, NG_GLEVELS, true), true);
    show("kdt_prof", kdt, 10, 512, false, LDS64K, knobs(0, NG_GLEVELS, true));

    const IterPlan it = plan_iter(512);
    printf("iter_mc512: ng=%d spt=%d dpq_alloc=%d vcap=%d\n", it.ng_cap, it.spt_cap,
           it.dpq_alloc, it.vcap);
    const IterPlan it2 = plan_iter(8192);
    printf("iter_mc8192: ng=%d spt=%d dpq_alloc=%d vcap=%d\n", it2.ng_cap, it2.spt_cap,
           it2.dpq_alloc, it2.vcap);
    printf("ref caps mc1: %d %d\n", ref_ng_cap(1), ref_spt_cap(1));
    return 0;
}

// TEST PROGRAM: prints the search launch plan (libbicos_amd/csrc/search_plan.cpp, linked alone:
// no kernel, no GPU) for the table of plan_cases.hpp, one line per case:
//   kind words bits cols rows nodupes keep row_valid keys T waves stream prune n:
// then per launch
//   family words ksteps nodupes T keys tail list agree stream prune lazy
//   @grid x block + lds bytes  chunk/tiles_per_row/tail_col0/tail_T;
// or "invalid" (hipErrorInvalidValue), or "unfusable" (search_mx_agree_fusable says no: no
// fused launch is asked for). tests/test_search_plan.py compares the output with
// tests/golden/search_plan.json.
#include "plan_cases.hpp"
#include "search_plan.hpp"

using namespace bicos_hip;

static void print_plan(const SearchLaunchPlan& p) {
    if (!p.ok) {
        std::printf(" invalid");
        return;
    }
    for (int i = 0; i < p.n; ++i) {
        const SearchLaunch& l = p.launch[i];
        const SearchVariant& v = l.v;
        const char* family = v.family == SearchFamily::mx ? "mx" : v.family == SearchFamily::pk ? "pk" : "lr";
        const bool pk = v.family == SearchFamily::pk;
        plan_cases::print_launch(family, v.words, pk ? 0 : v.ksteps, v.nodupes, v.T, v.keys, v.tail, v.list,
                                 v.agree, v.stream, v.prune, v.lazy, l.grid, l.block, (long)l.lds, l.chunk,
                                 l.tiles_per_row, l.tail_col0, l.tail_T);
    }
}

int main(int argc, char** argv) {
    static int16_t keep_dummy;
    static uint8_t valid_dummy;
    if (argc > 1) {  // the fused launch asked for with a (words, n) that is no fused shape
        SearchArgs a{};
        a.rows = 480;
        a.cols = 640;
        AgreeArgs ag{};
        int bad = 0;
        for (int words : {1, 2, 4, 8})
            for (int n : {8, 33}) {
                // the geometry of the shape that IS fusable at this n, the caller's width wrong
                const int w0 = n == 8 ? 1 : 4;
                const MxGeometry g = search_mx_geometry(a.rows, a.cols, w0, 64 * 1024, 0, 0, 256, 0, 29);
                ag.n = n;
                const bool ok = plan_search_mx(a, g, words, true, &ag).ok;
                std::printf("words %d n %d: %s\n", words, n, ok ? "planned" : "invalid");
                bad += ok != (words == w0);
            }
        return bad ? 1 : 0;
    }
    plan_cases::for_each_case([](const plan_cases::Case& c) {
        plan_cases::print_case(c);
        SearchArgs a{};
        a.rows = c.rows;
        a.cols = c.cols;
        a.keep = c.keep ? &keep_dummy : nullptr;
        a.row_valid = c.row_valid ? &valid_dummy : nullptr;
        if (c.kind == 'L') {
            print_plan(plan_search_lr(a, c.words, c.bits));
        } else {
            MxGeometry g = search_mx_geometry(c.rows, c.cols, c.words, 64 * 1024, c.T, c.waves, 256, c.keys, c.bits);
            g.stream = c.stream;
            g.prune = c.prune;
            AgreeArgs ag{};
            ag.n = c.n;
            if (c.kind == 'S')
                print_plan(plan_search_mx(a, g, c.words, c.nodupes != 0));
            else if (!search_mx_agree_fusable(g, c.words, true, c.cols, c.n, 1, false))
                std::printf(" unfusable");
            else
                print_plan(plan_search_mx(a, g, c.words, true, &ag));
        }
        std::printf("\n");
    });
    return 0;
}

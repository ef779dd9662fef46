// Host-side check of the call plan (csrc/rq_plan.h): the route, the cut into passes, the two scan grids and the non-temporal
// rule are plain arithmetic on the index's fields, so they run here on a default-constructed rq_index without a GPU and can be
// built with -fsanitize=address,undefined.  Every expectation was worked out by hand from the rules the header states.
//   hipcc -O1 -g -std=c++17 --offload-host-only -fsanitize=address,undefined -I <csrc> tests/native/plan_check.cpp -o plan_check
#include "rq_plan.h"

static thread_local char g_err[512] = "";
int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* rq_err_text() { return g_err; }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

static const unsigned DEFER8 = CALL_MAY_DEFER | CALL_ALLOW8;   // what rq_search_device passes
static const int64_t BIG = (int64_t)1 << 20;                   // 16384 bins: no default call is exact

static void fp16_index(rq_index& idx, int64_t n) { idx.dim = 768; idx.dpad = 768; idx.n = idx.cap = n; }
static void narrow_index(rq_index& idx, int64_t n) { idx.dim = 384; idx.dpad = 384; idx.n = idx.cap = n; }

static std::string passes_text(const CallPlan& p) {
    std::string s;
    for (int i = 0; i < p.npass; ++i) s += (i ? "," : "") + std::to_string(p.pass_q[i]);
    return s;
}
// the plan of a k = 10 call at the default nb
static CallPlan plan(const rq_index& idx, int B, bool use8, int k = 10, unsigned flags = DEFER8) {
    CallPlan p;
    const int r = plan_call(&idx, B, k, RQ_METRIC_COSINE, nb_default(&idx, k), use8, flags, &p);
    CHECK(r == RQ_OK, "plan_call(B=%d, k=%d) failed: %s", B, k, rq_err_text());
    return p;
}
static void check_passes(const rq_index& idx, int B, bool use8, const char* want, int want_split = -1) {
    const CallPlan p = plan(idx, B, use8);
    int sum = 0;
    for (int i = 0; i < p.npass; ++i) sum += p.pass_q[i];
    CHECK(passes_text(p) == want, "B=%d use8=%d wide_batch=%d dpad=%d: passes [%s], expected [%s]", B, (int)use8, idx.wide_batch, idx.dpad, passes_text(p).c_str(), want);
    CHECK(p.bpad == sum && p.bpad >= B, "B=%d: bpad %d, passes sum to %d", B, p.bpad, sum);
    if (want_split >= 0) CHECK(p.nwg_split == want_split, "B=%d use8=%d dpad=%d [%s]: nwg_split %d, expected %d", B, (int)use8, idx.dpad, want, p.nwg_split, want_split);
}

// `plan_check plan ROWS:DPAD:B:M:USE8 ...`: one line per shape with what plan_call decides for a search of B queries for M rows at
// the default nb on a default index of ROWS rows of DPAD elements -- "ROWS DPAD B M USE8 exact fast nb npass pass,pass,... wanted8".
// tests/test_route_shapes.py compares the lines with tests/route_shapes.py, the Python restatement the GPU tests rely on.
static int print_plans(int argc, char** argv) {
    for (int i = 2; i < argc; ++i) {
        long long rows = 0;
        int dpad = 0, B = 0, m = 0, use8 = 0;
        if (std::sscanf(argv[i], "%lld:%d:%d:%d:%d", &rows, &dpad, &B, &m, &use8) != 5 || (dpad != 768 && dpad != 384)) {
            std::printf("bad shape %s\n", argv[i]);
            return 2;
        }
        rq_index idx;
        if (dpad == 384) narrow_index(idx, rows); else fp16_index(idx, rows);
        CallPlan p;
        if (plan_call(&idx, B, m, RQ_METRIC_COSINE, nb_default(&idx, m), use8 != 0, CALL_ALLOW8, &p) != RQ_OK) {
            std::printf("plan_call(%s) failed: %s\n", argv[i], rq_err_text());
            return 2;
        }
        idx.scan8 = 2;                                             // ... and whether "scan8" = 2 would make the image the operand
        const int wanted8 = (int)scan8_wanted(&idx, B, m, nb_default(&idx, m), CALL_ALLOW8);
        std::printf("%lld %d %d %d %d %d %d %d %d %s %d\n", rows, dpad, B, m, use8, (int)p.exact, (int)p.fast, p.nb, p.npass, passes_text(p).c_str(), wanted8);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "plan") return print_plans(argc, argv);
    {   // ---- pass cutting and nwg_split --------------------------------------------------------------------------
        rq_index idx;
        fp16_index(idx, BIG);
        CHECK(idx.wide_batch == 1 && idx.wide256_8 == 31, "defaults moved");
        check_passes(idx, 64, false, "64", 0);
        check_passes(idx, 65, false, "128");
        check_passes(idx, 129, false, "256");
        check_passes(idx, 257, false, "256,64", 256);
        check_passes(idx, 320, false, "256,64");
        check_passes(idx, 384, false, "256,128");
        check_passes(idx, 385, false, "256,256", 512);
        idx.wide_batch = 3;
        check_passes(idx, 129, false, "128,64");
        idx.wide_batch = 0;
        check_passes(idx, 129, false, "64,64,64");
        CallPlan cap = plan(idx, 65535, false);                    // the cap itself is not an error
        CHECK(cap.npass == 1024 && cap.bpad == 65536, "B=65535 at wide_batch 0: %d passes", cap.npass);
        CHECK(plan_call(&idx, 65537, 10, RQ_METRIC_COSINE, 18, false, DEFER8, &cap) == RQ_EINVAL && std::string(rq_err_text()) == "too many passes",
              "1025 passes: %s", rq_err_text());
        idx.wide_batch = 1;                                        // the int8 image
        check_passes(idx, 65, true, "128");
        check_passes(idx, 300, true, "256,64");
        check_passes(idx, 384, true, "256,128", 256);
        idx.wide256_8 = 0;
        check_passes(idx, 130, true, "128,128");
        rq_index nar;
        narrow_index(nar, BIG);
        CHECK(nar.narrow() && plan(nar, 129, false).narrow, "narrow layout");
        check_passes(nar, 129, false, "128,64", 0);
        nar.wide_batch = 0;
        check_passes(nar, 129, false, "64,64,64");
    }
    {   // ---- exact route, nb, m, stride, grid ----------------------------------------------------------------------
        rq_index idx;
        fp16_index(idx, 2304);                                     // 36 bins
        CHECK(nb_default(&idx, 10) == 18, "nb_default(10) = %d", nb_default(&idx, 10));
        CallPlan p = plan(idx, 64, false);
        CHECK(p.exact && p.nb == 36 && !p.fast && p.ncand == 36 * 64, "n=2304: exact %d nb %d fast %d ncand %lld", (int)p.exact, p.nb, (int)p.fast, (long long)p.ncand);
        idx.n = 2305;                                              // 37 bins
        p = plan(idx, 64, false);
        CHECK(!p.exact && p.nb == 18 && p.m == 19 && p.stride == 64 && p.nquads == 37 && p.nbins == 37 && p.grid_wide == 37,
              "n=2305: exact %d nb %d m %d stride %lld nquads %d grid_wide %d", (int)p.exact, p.nb, p.m, (long long)p.stride, p.nquads, p.grid_wide);
        idx.n = BIG;
        CHECK(plan_call(&idx, 64, 10, RQ_METRIC_COSINE, -1, false, CALL_ALLOW8, &p) == RQ_OK && p.exact && p.nb == 16384 && p.m == 16385, "nb=-1: exact %d nb %d", (int)p.exact, p.nb);
        CHECK(plan_call(&idx, 64, 10, RQ_METRIC_COSINE, 3072, false, DEFER8, &p) == RQ_EINVAL && std::string(rq_err_text()) == "nb 3072 too large", "nb=3072: %s", rq_err_text());
        CHECK(plan_call(&idx, 64, 10, RQ_METRIC_COSINE, 3071, false, DEFER8, &p) == RQ_OK && !p.exact && p.nb == 3071, "nb=3071");
        p = plan(idx, 64, false);
        CHECK(p.stride == 16384 && p.grid_wide == 256, "1M rows: stride %lld grid_wide %d", (long long)p.stride, p.grid_wide);
        idx.max_sub_rel = 0.06;                                    // fp16-subnormal rows: the fp16 scan says nothing, the int8 image still does
        CHECK(scan_eps(&idx, RQ_METRIC_COSINE) > RQ_EPS_USELESS && plan(idx, 64, false).exact && !plan(idx, 64, true).exact, "subnormal shard");
    }
    {   // ---- fast tail ---------------------------------------------------------------------------------------------------
        rq_index idx;
        fp16_index(idx, BIG);
        CallPlan p = plan(idx, 64, false, 320);
        CHECK(p.fast && p.ncand == 4096, "k=320: fast %d ncand %lld", (int)p.fast, (long long)p.ncand);
        p = plan(idx, 64, false, 321);                             // nb = 321 + 321 / 8
        CHECK(!p.fast && p.nb == 361 && p.ncand == 361 * 64, "k=321: fast %d nb %d ncand %lld", (int)p.fast, p.nb, (long long)p.ncand);
        p = plan(idx, 64, false, 10, CALL_FORCE_GENERIC | CALL_ALLOW8);
        CHECK(!p.fast && p.ncand == 18 * 64, "force_generic: fast %d ncand %lld", (int)p.fast, (long long)p.ncand);
        idx.fast_tail = 0;
        CHECK(!plan(idx, 64, false).fast, "fast_tail = 0");
        // a wide pass leaves one partition maximum per workgroup, 256 of them: beyond 256 wanted rows the m-th largest does not exist
        idx.fast_tail = 1;
        CHECK(idx.cu_count == 256 && plan(idx, 130, false, 256).fast && plan(idx, 65, false, 256).fast && plan(idx, 300, false, 256).fast, "k = 256 on the wide grid");
        p = plan(idx, 130, false, 257);                            // nb = 257 + 257 / 8
        CHECK(!p.fast && !p.exact && p.nb == 289 && p.ncand == 289 * 64 && p.nwg_split == 256, "B=130 k=257: fast %d nb %d ncand %lld", (int)p.fast, p.nb, (long long)p.ncand);
        CHECK(!plan(idx, 65, false, 320).fast && !plan(idx, 300, false, 320).fast && plan(idx, 64, false, 320).fast, "k = 320: the 64-query grid alone holds 320 maxima");
        idx.wide_batch = 0;
        CHECK(plan(idx, 300, false, 320).fast, "passes of 64 only");
        idx.wide_batch = 1;
        idx.cu_count = 304;                                        // grid_wide 304
        CHECK(plan(idx, 130, false, 304).fast && !plan(idx, 130, false, 305).fast, "304 CUs");
        idx.cu_count = 256;
        CHECK(plan(idx, 130, true, 320).fast && plan(idx, 300, true, 257).fast, "the int8 image is read by the fast tail only: left to its ladder");
        rq_index nar;
        narrow_index(nar, BIG);
        CHECK(plan(nar, 200, false, 320).fast, "rows of 384 elements: no wide grid");
        rq_index small;
        fp16_index(small, 49157);                                  // 769 bins
        CHECK(plan(small, 130, false, 256).fast && !plan(small, 130, false, 257).fast && !plan(small, 130, false, 257).exact, "769 bins");
    }
    {   // ---- non-temporal loads: rows x scanned bytes per row beyond 208 MiB ----------------------------------------------
        rq_index idx;
        fp16_index(idx, 141994);
        CHECK(idx.nt == -1 && !plan(idx, 64, false).nt, "fp16 rows, n=141994");
        idx.n = 141995;
        CHECK(plan(idx, 64, false).nt && plan(idx, 64, false).scan_rowb == 1536, "fp16 rows, n=141995");
        CHECK(!plan(idx, 64, true).nt && plan(idx, 64, true).scan_rowb == 768, "int8 image, n=141995");
        idx.n = 283989;
        CHECK(!plan(idx, 64, true).nt, "int8 image, n=283989");
        idx.n = 283990;
        CHECK(plan(idx, 64, true).nt, "int8 image, n=283990");
        idx.nt = 0;
        CHECK(!plan(idx, 64, true).nt && !plan(idx, 64, false).nt, "nt = 0");
        idx.nt = 1; idx.n = 4096;
        CHECK(plan(idx, 64, false).nt, "nt = 1");
        rq_index nar;
        narrow_index(nar, 283989);
        CHECK(!plan(nar, 64, false).nt && plan(nar, 64, false).scan_rowb == 768, "narrow rows, n=283989");
        nar.n = 283990;
        CHECK(plan(nar, 64, false).nt, "narrow rows, n=283990");
    }
    {   // ---- the int8 decision and split8 ----------------------------------------------------------------------------------
        rq_index idx;
        fp16_index(idx, BIG);
        CHECK(idx.scan8 == 1 && idx.scan8_level[0] == 0 && idx.scan8_level[1] == 1, "defaults moved");
        CHECK(!plan(idx, 64, true, 10).split8 && plan(idx, 64, true, 100).split8, "split8 by class: one image for k <= 32, two beyond");
        CHECK(plan(idx, 64, true, 100).kclass == 1 && plan(idx, 64, true, 32).kclass == 0, "kclass");
        CHECK(!plan(idx, 65, true, 100).split8, "split8 at B = 65");
        CHECK(!plan(idx, 64, false, 100).split8, "split8 without use8");
        idx.scan8_level[1] = 0;
        CHECK(!plan(idx, 64, true, 100).split8, "split8 at level 0");
        idx.scan8_level[1] = 1;
        CHECK(scan8_wanted(&idx, 64, 10, 18, DEFER8) && scan8_wanted(&idx, 64, 128, 144, DEFER8), "wanted at 1M rows");
        CHECK(!scan8_wanted(&idx, 64, 10, 18, CALL_MAY_DEFER), "not allowed");
        CHECK(!scan8_wanted(&idx, 64, 10, 18, DEFER8 | CALL_FORCE_GENERIC), "generic tail");
        CHECK(!scan8_wanted(&idx, 64, 129, 145, DEFER8), "automatic rule: k <= 128");
        CHECK(!scan8_wanted(&idx, 64, 10, -1, DEFER8) && !scan8_wanted(&idx, 64, 10, 8192, DEFER8), "exact calls");
        idx.n = 99999;
        CHECK(!scan8_wanted(&idx, 64, 10, 18, DEFER8), "automatic rule: 100000 rows");
        idx.scan8 = 2;
        CHECK(scan8_wanted(&idx, 64, 10, 18, DEFER8) && scan8_wanted(&idx, 64, 320, 360, DEFER8) && !scan8_wanted(&idx, 64, 321, 361, DEFER8), "scan8 = 2");
        idx.scan8 = 0;
        CHECK(!scan8_wanted(&idx, 64, 10, 18, DEFER8), "scan8 = 0");
        idx.scan8 = 1; idx.n = BIG;
        CHECK(scan8_wanted(&idx, 65, 10, 18, DEFER8), "wide call, class at one image");
        idx.wide8 = 0;
        CHECK(!scan8_wanted(&idx, 65, 10, 18, DEFER8) && scan8_wanted(&idx, 64, 10, 18, DEFER8), "wide8 = 0");
        idx.wide8 = 1;
        CHECK(!scan8_usable(&idx, 64, 10), "no image built");
        rq_index nar;
        narrow_index(nar, BIG);
        CHECK(!scan8_wanted(&nar, 64, 10, 18, DEFER8), "narrow rows have no int8 image");
    }
    {   // ---- queries per group: as many as keep keys_per_query 8-byte keys each within 1 GiB (2^27 keys), in 1..B -------------------
        CHECK(queries_per_gib(64, 0) == 64 && queries_per_gib(64, 1) == 64 && queries_per_gib(65535, 1) == 65535, "0 or 1 key per query: the whole batch");
        CHECK(queries_per_gib(64, (int64_t)1 << 27) == 1 && queries_per_gib(64, ((int64_t)1 << 27) - 1) == 1 && queries_per_gib(64, (int64_t)1 << 26) == 2, "the quotient is exactly 1, then 2");
        CHECK(queries_per_gib(1, ((int64_t)1 << 27) + 64) == 1 && queries_per_gib(64, (int64_t)1 << 31) == 1, "one query beyond 1 GiB still runs, alone");
        CHECK(queries_per_gib(3, 1000) == 3 && queries_per_gib(1, 1) == 1, "B below the quotient");
        CHECK(queries_per_gib(65535, 4160) == 32263 && queries_per_gib(500, (1000000 + 63) / 64 * 64) == 134, "4 101 rows padded to 4 160 keys; 1M rows");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}

// Host-side soundness check of the certificate's last step, rq_certified (csrc/rq_device.h; compiled with hipcc, runs without a
// GPU).  rq_final_kernel (rq_select.hip) and rq_final_body.h both call it: b is the best approximate score a row that was not
// re-scored can have, and the answer may only be "certified" when NO such row can reach the k-th exact score s_k.
//
// SOUNDNESS: whenever rq_certified says yes, the bound evaluated in long double WITHOUT any slack factor --
//   cosine  b + eps          inner product  (b + eps * max_row_norm) * qn
// -- is strictly below s_k.  The sweep puts s_k on and within a few ulps of the bound, on both sides, for bounds of both signs.
// The reverse (no needless refusal) is checked loosely: a bound more than 4e-6 relative (and one fp32 ulp) below s_k certifies.
#include "rq_device.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int fails = 0;
static long checked = 0, yes = 0, yes_negative = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

static long double exact_bound(float b, float eps, float mrn, double qn, int metric) {
    const long double v = (long double)b + (long double)eps * (long double)(metric == 0 ? 1.f : mrn);
    return metric == 0 ? v : v * (long double)qn;
}

static void one(float b, float eps, float mrn, double qn, int metric, float sk) {
    const bool cert = rq_certified((double)b, eps, mrn, qn, metric, sk);
    const long double bound = exact_bound(b, eps, mrn, qn, metric);
    ++checked;
    if (cert) {
        ++yes;
        if (bound < 0) ++yes_negative;
        CHECK(bound < (long double)sk, "certified although the bound reaches s_k: metric %d b=%.9g eps=%.9g mrn=%.9g qn=%.17g bound=%.21Lg s_k=%.9g",
              metric, b, eps, mrn, qn, bound, sk);
    } else {
        const long double gap = (long double)sk - bound;
        CHECK(!(gap > 4e-6L * fabsl(bound) + (long double)std::fabs(sk) * 1.2e-7L + 1e-37L),
              "refused although the bound is far below s_k: metric %d b=%.9g eps=%.9g mrn=%.9g qn=%.17g bound=%.21Lg s_k=%.9g", metric, b, eps, mrn, qn, bound, sk);
    }
}

int main() {
    std::mt19937_64 rng(20261);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const float inf = std::numeric_limits<float>::infinity();
    const std::vector<float> epss = {0.f, 7.0e-4f, 7.3e-4f, 2.1e-3f, 10.f};
    const std::vector<float> mrns = {1.000001f, 0.5f, 2.000002f, 37.5f, 1e-3f};
    const std::vector<double> qns = {1.0, 3.0, 2.5, 0.1, 1e-3, 27.712812921102035, 1e4, 2e-17};
    std::vector<float> bs = {-1.f, -0.5f, -0.05f, -1e-3f, -7.0e-4f, -7.3e-4f, -1e-6f, 0.f, 1e-6f, 1e-3f, 0.05f, 0.5f, 0.999f, 1.f, -2.f, -65504.f, 65504.f};
    for (int i = 0; i < 4000; ++i) {
        bs.push_back((float)(-1.2 * U(rng)));                         // negative bounds: two in three
        bs.push_back((float)(-0.01 * U(rng)));
        bs.push_back((float)(1.2 * U(rng)));
    }
    for (int metric = 0; metric < 2; ++metric)
        for (float b : bs) {
            const float eps = epss[rng() % epss.size()], mrn = mrns[rng() % mrns.size()];
            const double qn = metric == 0 ? 1.0 : qns[rng() % qns.size()];
            const long double bound = exact_bound(b, eps, mrn, qn, metric);
            // s_k: the fp32 neighbours of the bound (8 ulps to each side), then 1e-7 .. 1e-4 relative to each side, then far away
            float c = (float)bound;
            float lo = c, hi = c;
            one(b, eps, mrn, qn, metric, c);
            for (int u = 0; u < 8; ++u) {
                lo = std::nextafter(lo, -inf); hi = std::nextafter(hi, inf);
                one(b, eps, mrn, qn, metric, lo);
                one(b, eps, mrn, qn, metric, hi);
            }
            for (double r : {1e-7, 5e-7, 9e-7, 1e-6, 1.1e-6, 2e-6, 4.1e-6, 1e-5, 1e-4, 0.5})
                for (double sgn : {-1.0, 1.0}) one(b, eps, mrn, qn, metric, (float)((double)bound + sgn * r * std::fabs((double)bound)));
            one(b, eps, mrn, qn, metric, 0.f);
            one(b, eps, mrn, qn, metric, -0.f);
            one(b, eps, mrn, qn, metric, inf);
            one(b, eps, mrn, qn, metric, -inf);
        }
    // the case of the analysis: an exact inner-product bound of -1 and s_k half a part in a million below it must not certify
    CHECK(!rq_certified(-1.0, 0.f, 1.f, 1.0, 1, -1.0000005f), "bound -1, s_k -1.0000005 certified");
    CHECK(rq_certified(-1.0, 0.f, 1.f, 1.0, 1, -0.99999f) && rq_certified(1.0, 0.f, 1.f, 1.0, 1, 1.00001f) && !rq_certified(1.0, 0.f, 1.f, 1.0, 1, 1.0000005f), "plain cases");
    // a non-negative bound keeps the expression it always had, bit for bit
    for (int i = 0; i < 100000; ++i) {
        const float b = (float)(1.2 * U(rng) - 0.0005), eps = epss[rng() % 4], mrn = mrns[rng() % mrns.size()];
        const double qn = qns[rng() % qns.size()];
        const double v = ((double)b + (double)eps * (double)mrn) * qn;
        if (!(v >= 0)) continue;
        const float was = (float)(v * (1.0 + 1e-6));
        for (float sk : {was, std::nextafter(was, inf), std::nextafter(was, -inf)})
            CHECK(rq_certified((double)b, eps, mrn, qn, 1, sk) == (was < sk), "b=%.9g eps=%.9g mrn=%.9g qn=%.17g", b, eps, mrn, qn);
    }
    CHECK(yes > checked / 8 && yes_negative > checked / 32, "the sweep certifies too rarely to say anything: %ld of %ld, %ld negative", yes, checked, yes_negative);
    std::printf("%s: %ld cases, %ld certified (%ld with a negative bound), %d failures\n", fails ? "FAILED" : "ok", checked, yes, yes_negative, fails);
    return fails ? 1 : 0;
}

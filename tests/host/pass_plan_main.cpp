// Checks the plan of the coordinate-descent passes (cnmf_amd/csrc/pass_plan.h) without a device
// (tests/test_host_pass_plan.py compiles this with the address and undefined-behaviour sanitizers and runs it).
//
//   pass_plan_main check      hand-derived expectations
//   pass_plan_main golden     every planner over the shape x knob grid, as JSON (compared with tests/golden/pass_plans.json)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>

#include "../../cnmf_amd/csrc/pass_plan.h"

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static const int SHAPES[] = {256, 512, 2048, 50176, 1100032};
static const int WIDTHS[] = {32, 64, 128, 256, 512, 1024};

// ------------------------------------------------------------------ stream-K plans
// Walk the P workgroups' unit ranges [U p / P, U (p + 1) / P) over the tiles in the order the kernels visit them and count,
// per tile, the boundaries that fall strictly inside it.
static std::vector<int> boundaries_per_tile(int T, int units, int P)
{
    std::vector<int> n(T, 0);
    const long long U = (long long)T * units;
    long long covered = 0;
    for (int p = 0; p < P; ++p) {
        const long long b = U * p / P, e = U * (p + 1) / P;
        CHECK(b == covered);                         // the ranges tile [0, U) exactly once, in order
        covered = e;
        if (p > 0 && b % units) ++n[b / units];
    }
    CHECK(covered == U);
    return n;
}

static void check_streamk3()
{
    const PadShape c3{50176, 2048};
    for (int KC : {256, 1024})
        for (int unit : {1, 2}) {
            const StreamK3 sk = plan_streamk3(KC, c3, 256, PLAN_G3C_JW, unit, false);
            CHECK(sk.on);
            CHECK(sk.MG == KC / 256 && sk.T == sk.MG * (50176 / 256) && sk.Kb == 2048 / (16 * unit) && sk.P == 256);
            CHECK((int)sk.flags.size() == sk.T);
            const std::vector<int> nb = boundaries_per_tile(sk.T, sk.Kb, sk.P);
            const int NJ = sk.T / sk.MG;
            for (int o = 0; o < sk.T; ++o) {        // o = mg * NJ + jt, the kernels' order; the sweep reads jt * MG + mg
                const int mg = o / NJ, jt = o % NJ, f = sk.flags[jt * sk.MG + mg];
                CHECK(f == 0 || f == 1 || f == 3);
                CHECK(f == (nb[o] == 0 ? 0 : (nb[o] == 1 ? 1 : 3)));
                CHECK(nb[o] <= 2);                   // a third boundary in one tile would have no plane to go to
            }
        }
    // off: fewer tiles than 3/4 of the workgroups, more than two workgroups per tile, the knob
    CHECK(!plan_streamk3(256, PadShape{256 * 191, 2048}, 256, 256, 1, false).on);      // T = 191 < 192
    CHECK(plan_streamk3(256, PadShape{256 * 192, 2048}, 256, 256, 1, false).on);
    CHECK(!plan_streamk3(256, PadShape{256, 2048}, 3, 256, 1, false).on);              // T = 1 >= 3/2 + 3/4, but P = 3 > 2 T
    CHECK(plan_streamk3(256, PadShape{256, 2048}, 2, 256, 1, false).on);
    CHECK(!plan_streamk3(256, c3, 256, 256, 1, true).on);
    CHECK(plan_streamk3(256, c3, 256, 256, 1, true).flags.empty());
}

static void check_streamk()
{
    const PadShape c3{50176, 2048};
    for (int KC : {128, 256}) {
        const StreamK sk = plan_streamk(KC, c3, 512, false);
        CHECK(sk.on && sk.MG == KC / 128 && sk.T == sk.MG * 392 && sk.nk == 64 && sk.P == (KC == 128 ? 256 : 512));    // 392 tiles <= 512: one workgroup per CU
        const std::vector<int> nb = boundaries_per_tile(sk.T, sk.nk, sk.P);
        for (int t = 0; t < sk.T; ++t) { CHECK(nb[t] <= 1); CHECK(sk.split[t] == nb[t]); }
    }
    CHECK(!plan_streamk(64, c3, 512, false).on);                                // KC % 128
    CHECK(!plan_streamk(128, PadShape{128 * 200, 2048}, 512, false).on);        // T = 200 <= P = 256 after halving
    CHECK(!plan_streamk(128, PadShape{128 * 1024, 2048}, 512, false).on);       // T % P == 0
    CHECK(!plan_streamk(128, c3, 512, true).on);                                // the knob
}

// ------------------------------------------------------------------ split counts
static void check_splits()
{
    for (int Kb = 1; Kb <= 4096; ++Kb)
        for (int n = 1; n <= 64; ++n)
            for (int nsub : {1, 2}) CHECK(gemm2h_splits(Kb, n, nsub) <= n && gemm2h_splits(Kb, n, nsub) >= 1);
    for (int K = 32; K <= 8192; K += 32)
        for (int n = 1; n <= 64; ++n) CHECK(effective_splits(K, n) <= n && effective_splits(K, n) >= 1);
    // no planned launch writes more partial planes than ensure_batch sized (size_splits), at the width allocated and
    // at every narrower width compact() re-plans at with the buffers' planes re-cut (cap * KC0 / KC)
    for (int N_pad : SHAPES) for (int G_pad : SHAPES) for (int KC0 : WIDTHS)
        for (int gemm3 : {1, 4}) for (int wgk : {0, 32, 128}) for (int nsk = 0; nsk < 2; ++nsk) for (int use3 = 0; use3 < 2; ++use3) {
            const PadShape s{N_pad, G_pad};
            if (use3 && (KC0 % 256 || N_pad % 128 || G_pad % 128)) continue;
            const int wg = gemm3_wg_slots(gemm3, wgk);
            const SplitCaps caps = size_splits(s, KC0, use3, wg);
            CHECK(caps.nsplit >= 1 && caps.nsplitA >= 1);
            for (int KC = KC0; KC >= (use3 ? 256 : KC0); KC -= 256)
                for (int jw : {PLAN_G3_JW, PLAN_G3C_JW}) for (int nsub : {1, 2}) {
                    if (jw == PLAN_G3C_JW && (N_pad % 256 || G_pad % 256)) continue;
                    if (nsub == 2 && ((G_pad / 16) % 2 || !use3)) continue;
                    const int cap = caps.nsplit * KC0 / KC, capA = caps.nsplitA * KC0 / KC;
                    PassPlan p;
                    plan_pass_splits(p, s, KC, use3, jw, nsub, wg, nsk, cap, capA);
                    if (use3) {
                        // pass B grid.z of launch_gemm3 / launch_gemm3c / the f16 launch with whole steps
                        const int Kb = N_pad / 16, kb_per = (Kb + p.nsplit3 - 1) / p.nsplit3;
                        CHECK((Kb + kb_per - 1) / kb_per <= cap);
                        CHECK(gemm2h_splits(Kb, p.nsplit3, gemm2h_nsub(false, Kb, nsub)) <= cap);
                        if (!p.sk3.on) {
                            const int KbA = G_pad / 16, ka = (KbA + p.nsplitA - 1) / p.nsplitA;
                            CHECK((KbA + ka - 1) / ka <= capA);
                            CHECK(gemm2h_splits(KbA, p.nsplitA, nsub) <= capA);
                        }
                    } else {
                        CHECK(p.nsplit <= cap);            // launch_gemm<true>: grid.z = nsplit
                        CHECK(p.nsplitA <= capA);          // launch_gemm<false>: grid.z = nsplitA (1 under stream-K)
                    }
                }
        }
}

// ------------------------------------------------------------------ the selectors
// the two ladders of the parent's launch_gemm2h / launch_gemm2h_streamk, typed out: {NSUB, HI, VAR, NTB, PART, GEN}
struct Key { int NSUB, HI, VAR, NTB, PART, GEN; };
static bool ladder_ksplit(bool Bhi, bool cscale, bool gen4, int gvar, int nsub, bool part, Key* k)
{
    if (Bhi && cscale && !gen4) {
        if (gvar == 0) { *k = part ? Key{1, 1, 0, 0, 1, 1} : Key{1, 1, 0, 0, 0, 1}; return true; }
        *k = part ? Key{1, 1, 4, 0, 1, 1} : Key{1, 1, 4, 0, 0, 1}; return true;
    }
    if (Bhi) { *k = part ? Key{1, 1, 0, 0, 1, 0} : Key{1, 1, 0, 0, 0, 0}; return true; }
    if (cscale) return false;
    if (nsub == 2) { *k = part ? Key{2, 0, 4, 0, 1, 0} : Key{2, 0, 4, 0, 0, 0}; return true; }
    *k = Key{1, 0, 4, 0, 0, 0}; return true;
}
static bool ladder_streamk(bool Bhi, bool cscale, bool gen4, int gvar, int nsub, bool part, bool shared, Key* k)
{
    if (Bhi && cscale && !gen4) {
        if (gvar == 0) {
            if (part) { *k = Key{1, 1, 0, 0, 1, 1}; return true; }
            *k = shared ? Key{1, 1, 0, 0, 0, 1} : Key{1, 1, 0, 1, 0, 1}; return true;
        }
        if (part) { *k = Key{1, 1, 4, 0, 1, 1}; return true; }
        *k = shared ? Key{1, 1, 4, 0, 0, 1} : Key{1, 1, 4, 1, 0, 1}; return true;
    }
    if (Bhi) {
        if (part) { *k = Key{1, 1, 0, 0, 1, 0}; return true; }
        *k = shared ? Key{1, 1, 0, 0, 0, 0} : Key{1, 1, 0, 1, 0, 0}; return true;
    }
    if (cscale) return false;
    if (nsub == 2) {
        if (part) { *k = Key{2, 0, 4, 0, 1, 0}; return true; }
        *k = shared ? Key{2, 0, 4, 0, 0, 0} : Key{2, 0, 4, 1, 0, 0}; return true;
    }
    *k = shared ? Key{1, 0, 4, 0, 0, 0} : Key{1, 0, 4, 1, 0, 0}; return true;
}

static void check_g2_form()
{
    typedef std::tuple<int, int, int, int, int, int> Tup;
    std::set<Tup> ks, sk;
    int n = 0;
    for (int hi = 0; hi < 2; ++hi) for (int gen = 0; gen < 2; ++gen) for (int gen4 = 0; gen4 < 2; ++gen4)
        for (int gvar : {0, 4}) for (int nsub : {1, 2}) for (int part = 0; part < 2; ++part) for (int shared = 0; shared < 2; ++shared) {
            ++n;
            const G2Form f = g2_form(hi, gen, gen4, gvar, nsub, part, shared);
            Key a{}, b{};
            const bool va = ladder_ksplit(hi, gen, gen4, gvar, nsub, part, &a), vb = ladder_streamk(hi, gen, gen4, gvar, nsub, part, shared, &b);
            CHECK(f.valid == va && f.valid == vb);
            CHECK(f.valid == !(gen && !hi));
            if (!f.valid) continue;
            CHECK(f.NSUB == a.NSUB && f.HI == (bool)a.HI && f.VAR == a.VAR && f.PART == (bool)a.PART && f.GEN == (bool)a.GEN);
            CHECK(f.NSUB == b.NSUB && f.HI == (bool)b.HI && f.VAR == b.VAR && f.NTB == (bool)b.NTB && f.PART == (bool)b.PART && f.GEN == (bool)b.GEN);
            if (!hi && nsub == 1) CHECK(!f.PART);            // the one-block count stream has no partial-tile form
            CHECK(g2_xmap(f, -1) == (f.GEN ? 0 : 1) && g2_xmap(f, 0) == 0 && g2_xmap(f, 1) == 1);
            ks.insert(Tup(f.NSUB, f.HI, f.VAR, 0, f.PART, f.GEN));
            sk.insert(Tup(f.NSUB, f.HI, f.VAR, f.NTB, f.PART, f.GEN));
        }
    CHECK(n == 128);
    CHECK(ks.size() == 9);
    CHECK(sk.size() == 14);
}

static void check_sweep_form()
{
    typedef SweepForm F;
    // [planes][psum][exact][a64]
    const F want[2][2][2][2] = {
        {{{F::W, F::W_A64}, {F::H_RMX, F::H_RMX}}, {{F::H_PSUM, F::H_PSUM}, {F::H_PSUM, F::H_PSUM}}},
        {{{F::W_PLN, F::W_PLN_A64}, {F::INVALID, F::INVALID}}, {{F::INVALID, F::INVALID}, {F::INVALID, F::INVALID}}}};
    for (int pl = 0; pl < 2; ++pl) for (int ps = 0; ps < 2; ++ps) for (int ex = 0; ex < 2; ++ex) for (int a = 0; a < 2; ++a) {
        CHECK(sweep_form(pl, ps, ex, a) == want[pl][ps][ex][a]);
        // tier 8 (ranks 65..128, sweep_big_kernel): never PSUM, never planes; the other forms are unchanged
        const F big = sweep_form(pl, ps, ex, a, 8 | 4);
        CHECK(big == ((pl || ps) ? F::INVALID : want[pl][ps][ex][a]));
    }
    CHECK(!sweep_a64(8388607) && sweep_a64(8388608));        // 64 * ldv * 4 against 2^31 - 1
    CHECK(!sweep_a64(1100032));
}

static void check_misc()
{
    CHECK(gemm3_wg_slots(4, 0) == 256 && gemm3_wg_slots(1, 0) == 512 && gemm3_wg_slots(4, 32) == 32 && gemm3_wg_slots(4, 31) == 256 &&
          gemm3_wg_slots(1, 128) == 512);
    CHECK(g2_full_mask(256) == 0xffull && g2_full_mask(1024) == 0xffffffffull && g2_full_mask(2048) == ~0ull);
    CHECK(gemm2h_nsub(false, 128, 2) == 2 && gemm2h_nsub(true, 128, 2) == 1 && gemm2h_nsub(false, 127, 2) == 1 && gemm2h_nsub(false, 128, 1) == 1);
    CHECK(sweep_chunks(64, 50000) == 4 && sweep_parts(64, 50000) == 49 && sweep_chunks(64, 100) == 1 && sweep_parts(64, 100) == 1);
    CHECK(split2h_wide(2048) && !split2h_wide(2112) && split2h_col_groups(2048, 256) == 8);
    CHECK(pick_kc(0, 1024, 1000, 10, 0, true) == 1024 && pick_kc(0, 1024, 1000, 10, 0, false) == 256 && pick_kc(0, 1024, 40, 9, 0, true) == 64 &&
          pick_kc(0, 1024, 5, 100, 0, false) == 128 && pick_kc(512, 1024, 1000, 10, 0, true) == 512);
}

// x_launches_fit at the grid limits of the launches it stands for (65 535 blocks on grid.y):
//   count detection, 256 rows per block   : 65 535 * 256 = 16 776 960 rows, the next padded shape is 16 777 216
//   bf16 plane split of X, 64 rows each   : 65 535 * 64  =  4 194 240 rows, the next shape of whole 128-row tiles 4 194 304
//   transposed builders, 256 genes each   : G_pad = 65 535 * 256, one tile more
static void check_launch_fit()
{
    const int G = 2048;
    // mode 4 on whole 256 x 256 tiles: the detection's chunks bound the rows (no launch of it carries rows / 64 on grid.y)
    CHECK(x_launches_fit(PadShape{16776960, G}, 4) && !x_launches_fit(PadShape{16777216, G}, 4));
    CHECK(x_launches_fit(PadShape{4194304, G}, 4));
    // modes 1 and 2 always split X into bf16 planes; mode 3 does when the matrix has no count structure
    for (int mode : {1, 2, 3}) CHECK(x_launches_fit(PadShape{4194240, G}, mode) && !x_launches_fit(PadShape{4194304, G}, mode));
    // mode 4 off the 256 grid has neither the count nor the general f16 path: the bf16 planes again
    CHECK(x_launches_fit(PadShape{4194240 - 128, G}, 4) && !x_launches_fit(PadShape{4194304 + 128, G}, 4));
    // the gene side rides on grid.y of every transposed builder, in every mode
    for (int mode : {1, 2, 3, 4}) {
        CHECK(x_launches_fit(PadShape{2048, 65535 * 256}, mode));
        CHECK(!x_launches_fit(PadShape{2048, 65535 * 256 + 128}, mode) && !x_launches_fit(PadShape{2048, 65536 * 256}, mode));
    }
    // nothing to launch on the f32 pipe; the shapes of the recorded plans all fit
    CHECK(x_launches_fit(PadShape{1 << 30, 1 << 30}, 0));
    for (int N_pad : SHAPES) for (int G_pad : SHAPES) for (int mode : {1, 2, 3, 4}) CHECK(x_launches_fit(PadShape{N_pad, G_pad}, mode));
}

// ------------------------------------------------------------------ golden
// FNV-1a over the integers of a plan and its cut flags: a record keeps one digest per group of stream-K plans
struct Fnv {
    unsigned long long h = 1469598103934665603ull;
    void byte(unsigned char c) { h ^= c; h *= 1099511628211ull; }
    void num(long long v) { for (int i = 0; i < 8; ++i) byte((unsigned char)((unsigned long long)v >> (8 * i))); }
    void bytes(const std::vector<unsigned char>& v) { num((long long)v.size()); for (unsigned char c : v) byte(c); }
};

static void golden()
{
    printf("{\"records\": [\n");
    bool first = true;
    for (int N_pad : SHAPES) for (int G_pad : SHAPES) for (int KC : WIDTHS) {
        const PadShape s{N_pad, G_pad};
        printf("%s{\"N_pad\": %d, \"G_pad\": %d, \"KC\": %d, ", first ? "" : ",\n", N_pad, G_pad, KC);
        first = false;
        printf("\"base\": [%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d], ", pick_nsplit(s, KC), pick_nsplit_A(s, KC),
               effective_splits(G_pad, 16), effective_splits(N_pad, 7), split2h_wide(G_pad), split2h_col_groups(G_pad, KC),
               split2h_col_groups(N_pad, KC), sweep_chunks(64, N_pad - 3), sweep_parts(64, N_pad - 3), sweep_chunks(5, G_pad - 3),
               sweep_parts(5, G_pad - 3), (int)(g2_full_mask(KC) % 1000003ull));
        printf("\"streamk\": [");                       // per no_streamk: on, cut tiles, digest of the whole plan
        for (int nsk = 0; nsk < 2; ++nsk) {
            const StreamK k = plan_streamk(KC, s, 512, nsk);
            Fnv f;
            for (int v : {(int)k.on, k.MG, k.T, k.nk, k.P, k.mw}) f.num(v);
            f.bytes(k.split);
            int cut = 0;
            for (unsigned char c : k.split) cut += c == 1;
            printf("%s%d, %d, \"%llx\"", nsk ? ", " : "", (int)k.on, cut, f.h);
        }
        printf("], \"slots\": [");
        bool f2 = true;
        for (int wgk : {0, 32, 128}) {
            const int wg = gemm3_wg_slots(4, wgk);
            const SplitCaps c0 = size_splits(s, KC, false, wg), c1 = size_splits(s, KC, true, wg);
            printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %d, ", f2 ? "" : ", ", wg, pick_nsplit3(s, KC, 128, wg), pick_nsplit3(s, KC, 256, wg),
                   pick_nsplit_A3(s, KC, 128, wg), pick_nsplit_A3(s, KC, 256, wg), c0.nsplit, c0.nsplitA, c1.nsplit, c1.nsplitA);
            f2 = false;
            // the eight plan_streamk3 of this slot count (no_streamk x tile width x g2_nsub): how many are on, cut tiles, one digest
            Fnv f;
            int on = 0, cut1 = 0, cut2 = 0;
            for (int nsk = 0; nsk < 2; ++nsk) for (int jw : {128, 256}) for (int nsubk : {1, 2}) {
                const int unit = gemm2h_nsub(false, G_pad / 16, nsubk);
                const StreamK3 k = plan_streamk3(KC, s, wg, jw, unit, nsk);
                for (int v : {unit, (int)k.on, k.T, k.Kb, k.P, k.MG}) f.num(v);
                f.bytes(k.flags);
                f.num(gemm2h_splits(N_pad / 16, pick_nsplit3(s, KC, jw, wg), gemm2h_nsub(false, N_pad / 16, nsubk)));
                on += k.on;
                for (unsigned char c : k.flags) { cut1 += c == 1; cut2 += c == 3; }
            }
            printf("%d, %d, %d, \"%llx\"]", on, cut1, cut2, f.h);
        }
        printf("]}");
    }
    printf("\n],\n\"wg_slots\": [");
    for (int g = 0; g <= 4; ++g) for (int w : {0, 31, 32, 128, 300}) printf("%s%d", (g || w) ? ", " : "", gemm3_wg_slots(g, w));
    printf("],\n\"pick_kc\": [");
    bool f4 = true;
    for (int kck : {0, 31, 64, 512}) for (int lim : {256, 1024, 2048}) for (long long tk : {1ll, 33ll, 200ll, 257ll, 900ll, 5000ll})
        for (int mk : {1, 40, 128}) for (int kcm : {0, 64, 300, 512, 4096}) for (int wide = 0; wide < 2; ++wide) {
            printf("%s%d", f4 ? "" : ", ", pick_kc(kck, lim, tk, mk, kcm, wide));
            f4 = false;
        }
    printf("]}\n");
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "golden")) { golden(); return 0; }
    if (argc != 2 || strcmp(argv[1], "check")) { fprintf(stderr, "usage: pass_plan_main check | golden\n"); return 2; }
    check_streamk3();
    check_streamk();
    check_splits();
    check_g2_form();
    check_sweep_form();
    check_misc();
    check_launch_fit();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}

// fusion_ledger_check.cpp — the step-fusion ledger (csrc/mg_fusion.h) checked on
// the host alone, against Isaac Gym's tensor contract.
//
// SEQUENCE LENGTH: every sequence of 5 calls (19^5 per configuration, 256
// configurations; prefixes are shared, so every shorter sequence is checked on
// the way): about 18 CPU-seconds, spread over up to 16 threads. 6 would take
// nineteen times as long.
//
// An abstract machine stands in for HIP. The device's root rows, other body
// rows, DOF state and first target column, each bound tensor, each other
// refresh destination, the host stage's parts and every set source hold an
// integer version; each answer of the ledger moves versions between them: a
// scatter or copy (source -> device), a step kernel (reads the device or a
// deferred source, writes the device and the outputs the ledger named), a
// gather (device -> destination). The truth is the contract run on the same
// integers: every set lands at its call, every refresh or fetch gathers, a
// simulate makes a new version from what it read. Sources are not modified
// while a set waits (that hazard is the Python layer's to catch), a discard
// makes the truth forget the sets it dropped, a rebind stands for "the caller
// wrote the bound tensors", and a fetch inside a capture is refused by the C
// ABI, so it is no call here.
//
// Enumerated: every sequence over the 19 calls below, under every combination
// of the five MG_FUSE_* bits, with and without bound tensors, with roots_free
// and step_writes_rows each true and false. Asserted at every call:
//   1. every value a reader observes (a refresh destination, a fetched part,
//      the state and targets a simulate starts from) is the truth's;
//   2. a simulate's kernels read a deferred set only if it was made under the
//      capture id the simulate runs under (any other was applied before, which
//      1. checks), and a set made eagerly that is applied inside a capture is
//      launched outside its graph, whose replays would apply it again;
//   3. with MG_FUSE_IN_CAPTURE off, inside a capture nothing is deferred, no
//      kernel reads a source or writes a bound tensor, no refresh is skipped;
//   4. a refresh is skipped only into a bound tensor that holds the current
//      state and was written it under the current capture id;
//   5. with all bits off no device set is deferred, no refresh is skipped or
//      paired and no kernel writes a bound tensor. (The CPU pipeline's mapped
//      input buffer and output stage are not fusion: they copy at the call and
//      serve only mg_fetch_host_state, under any flags.)
// Then the sequences include/migym.h documents. Exit status 0 and "0 failures"
// when all hold.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "mg_fusion.h"

enum Call {
    ROOT_DEV, ROOT_DEV_IDX, ROOT_HOST, RB_SET, DOF_SET, TGT_DEV, TGT_DEV_IDX, SIMULATE,
    REF_ROOT_BOUND, REF_RB_BOUND, REF_DOF_BOUND, REF_ROOT_OTHER, REF_RB_OTHER, REF_DOF_OTHER,
    FETCH, DISCARD, REBIND, CAPTURE_BEGINS, CAPTURE_ENDS, N_CALLS
};
static const char* const kCallName[N_CALLS] = {
    "root_dev", "root_dev_idx", "root_host", "rb_set", "dof_set", "tgt_dev", "tgt_dev_idx", "simulate",
    "ref_root_bound", "ref_rb_bound", "ref_dof_bound", "ref_root_other", "ref_rb_other", "ref_dof_other",
    "fetch", "discard", "rebind", "capture_begins", "capture_ends"};
constexpr int kLen = 5;
constexpr int kMaxLen = 24;   // the documented sequences are longer than kLen

struct Cfg {
    int flags;
    bool bound, roots_free, writes_rows;
};

// what the pointers handed to the ledger stand for
static float g_src[kMaxLen + 1];   // one source per call; the last: the mapped root input buffer
static float g_bound[MG_PART_N], g_other[MG_PART_N], g_stage[1];
static float* const kMapped = &g_src[kMaxLen];
constexpr uint32_t kGarbage = 0xdeadu;

static uint32_t mix(uint32_t a, uint32_t b, uint32_t c) { return (a * 0x9E3779B1u ^ b) * 0x85EBCA6Bu + c * 0xC2B2AE35u + 1u; }

struct World {
    MgFusion F;
    uint32_t tR = 1, tB = 2, tD = 3, tT = 4;      // truth: root rows, other body rows, DOF state, target column 0
    uint32_t mR = 1, mB = 2, mD = 3, mT = 4;      // the device's own
    uint32_t bt[MG_PART_N], ot[MG_PART_N], hs[MG_PART_N];
    uint8_t wcid[MG_PART_N][8];                   // the captures under which a bound tensor was written what it holds
    int nw[MG_PART_N];
    uint32_t srcv[kMaxLen + 1];                   // version each source holds
    uint8_t made[kMaxLen + 1];                    // capture each deferred source was set under
    unsigned long long cid = 0, ncap = 0;
    int n = 0;                                    // calls so far
    // of the last call, for the documented sequences
    int set_how = -1, refresh_how = -1, fetch_need = -1, sim_out = -1;
    bool sim_read_root = false, sim_read_tgt = false;
};

static std::atomic<int> failures{0};
struct Trace {
    const Cfg* cfg;
    int call[kMaxLen];
    int n;
};
static void report(const Trace& t, const char* what) {
    if (failures.fetch_add(1) >= 20) return;
    std::printf("FAIL %s: flags %d bound %d roots_free %d writes_rows %d:", what, t.cfg->flags, t.cfg->bound,
                t.cfg->roots_free, t.cfg->writes_rows);
    for (int i = 0; i < t.n; ++i) std::printf(" %s", kCallName[t.call[i]]);
    std::printf("\n");
}
#define CHECK(c, what)                 \
    do {                               \
        if (!(c)) report(t, what);     \
    } while (0)

static uint32_t part_truth(const World& w, int part) {
    return part == MG_PART_ROOT ? w.tR : part == MG_PART_RB ? mix(w.tR, w.tB, 7) : w.tD;
}
static uint32_t part_device(const World& w, int part) {
    return part == MG_PART_ROOT ? w.mR : part == MG_PART_RB ? mix(w.mR, w.mB, 7) : w.mD;
}
static uint32_t version(const World& w, const float* src) { return w.srcv[src - g_src]; }
// the ordinary launches the ledger asks for: a deferred set is always a full one
static void landed(const World& w, const Trace& t, const MgFusion::Apply& a) {
    CHECK(a.outside == (w.made[a.src - g_src] == 0 && w.cid != 0),
          "2: a set made eagerly is launched outside the graph of a later capture, and only such a set");
}
static void scatter_root(World& w, const Trace& t, const MgFusion::Apply& a) {
    if (!a.src) return;
    landed(w, t, a);
    w.mR = version(w, a.src);
}
static void copy_tgt(World& w, const Trace& t, const MgFusion::Apply& a) {
    if (!a.src) return;
    landed(w, t, a);
    w.mT = version(w, a.src);
}
// a launch under the current capture writes v into bound tensor `part`
static void write_bound(World& w, int part, uint32_t v) {
    if (w.bt[part] != v) w.nw[part] = 0;
    w.bt[part] = v;
    if (w.nw[part] < 8) w.wcid[part][w.nw[part]++] = (uint8_t)w.cid;
}
static bool written_here(const World& w, int part) {
    for (int i = 0; i < w.nw[part]; ++i)
        if (w.wcid[part][i] == w.cid) return true;
    return false;
}
static void rebind(World& w, const Cfg& c) {
    w.F.bind(c.bound ? &g_bound[MG_PART_ROOT] : nullptr, c.bound ? &g_bound[MG_PART_RB] : nullptr);
    w.F.bind_dof(c.bound ? &g_bound[MG_PART_DOF] : nullptr);
    for (int k = 0; k < MG_PART_N; ++k) {
        w.bt[k] = kGarbage;
        w.nw[k] = 0;
    }
}
static World make_world(const Cfg& c) {
    World w;
    w.F.set_flags(c.flags);
    for (int k = 0; k < MG_PART_N; ++k) w.ot[k] = w.hs[k] = kGarbage;
    rebind(w, c);
    return w;
}

static void set_checks(const World& w, const Cfg& c, const Trace& t, const MgFusion::Set& f, bool may_map) {
    const bool in_capture_off = w.cid != 0 && !(c.flags & MG_FUSE_IN_CAPTURE);
    CHECK(!(in_capture_off && f.how != MG_SET_NOW), "3: a set deferred inside a capture without MG_FUSE_IN_CAPTURE");
    CHECK(!(c.flags == 0 && f.how == MG_SET_DEFER), "5: a device set deferred with all bits off");
    CHECK(f.how != MG_SET_DEFER_MAPPED || may_map, "the mapped buffer is for full host root sets");
    CHECK(w.F.last_set_deferred == (f.how == MG_SET_DEFER), "mg_last_set_deferred is 1 exactly for a deferred device set");
}

static void refresh(World& w, const Cfg& c, const Trace& t, int part, bool into_bound) {
    if (part != MG_PART_DOF) scatter_root(w, t, w.F.read_state(w.cid));
    float* dst = into_bound ? &g_bound[part] : &g_other[part];
    uint32_t& held = into_bound ? w.bt[part] : w.ot[part];
    const MgFusion::Refresh r = w.F.refresh(part, dst, false, w.cid, true);
    w.refresh_how = r.how;
    if (r.how == MG_REFRESH_SKIP) {
        CHECK(!(w.cid != 0 && !(c.flags & MG_FUSE_IN_CAPTURE)), "3: a refresh skipped inside a capture without MG_FUSE_IN_CAPTURE");
        CHECK(c.flags != 0, "5: a refresh skipped with all bits off");
        CHECK(into_bound && c.bound, "4: a refresh skipped into a tensor that is not bound");
        CHECK(written_here(w, part), "4: a refresh skipped into a tensor that this capture did not write");
    } else if (r.how == MG_REFRESH_PAIRED) {
        CHECK(c.flags & MG_FUSE_REFRESH, "5: the paired gather without MG_FUSE_REFRESH");
        CHECK(part == MG_PART_ROOT && into_bound && c.bound && r.rb == &g_bound[MG_PART_RB], "the paired gather is the bound root refresh");
        write_bound(w, MG_PART_ROOT, w.mR);
        write_bound(w, MG_PART_RB, part_device(w, MG_PART_RB));
        w.F.refreshed(r, w.cid);
        CHECK(w.bt[MG_PART_RB] == part_truth(w, MG_PART_RB), "1: the paired rigid-body tensor");
    } else {
        if (into_bound) write_bound(w, part, part_device(w, part));
        else held = part_device(w, part);
        w.F.refreshed(r, w.cid);
    }
    CHECK(held == part_truth(w, part), "1: a refresh destination does not hold the state");
}

static void simulate(World& w, const Cfg& c, const Trace& t) {
    const MgFusion::Begin b = w.F.begin_simulate(w.cid, true, true);
    scatter_root(w, t, b.root);
    copy_tgt(w, t, b.tgt[0]);
    const MgFusion::Step p = w.F.step(w.cid, c.writes_rows);
    w.sim_out = p.out;
    w.sim_read_root = p.root_src != nullptr;
    w.sim_read_tgt = p.tgt[0] != nullptr;
    CHECK(!p.tgt[1] && !p.tgt[2], "a target column nobody set");
    CHECK(!p.root_src || w.made[p.root_src - g_src] == w.cid, "2: the step reads a root set of another capture");
    CHECK(!p.tgt[0] || w.made[p.tgt[0] - g_src] == w.cid, "2: the step reads a target set of another capture");
    if (w.cid != 0 && !(c.flags & MG_FUSE_IN_CAPTURE))
        CHECK(!p.root_src && !p.tgt[0] && p.out == MG_OUT_NONE, "3: a fused step inside a capture without MG_FUSE_IN_CAPTURE");
    if (c.flags == 0)
        CHECK((!p.root_src || p.root_src == kMapped) && !p.tgt[0] && p.out != MG_OUT_BOUND, "5: a fused step with all bits off");
    CHECK(p.out == MG_OUT_NONE || c.writes_rows, "step outputs from kernels that do not write rows");
    // the kernels: read the deferred sources in place of the device's own (the target is written through)
    const uint32_t R = p.root_src ? version(w, p.root_src) : w.mR;
    w.mT = p.tgt[0] ? version(w, p.tgt[0]) : w.mT;
    CHECK(R == w.tR && w.mB == w.tB && w.mD == w.tD && w.mT == w.tT, "1: the simulate starts from another state or target");
    const uint32_t h = mix(mix(R, w.mB, w.mD), w.mT, 11);
    w.mR = mix(h, 1, 0); w.mB = mix(h, 2, 0); w.mD = mix(h, 3, 0);
    const uint32_t ht = mix(mix(w.tR, w.tB, w.tD), w.tT, 11);
    w.tR = mix(ht, 1, 0); w.tB = mix(ht, 2, 0); w.tD = mix(ht, 3, 0);
    if (p.out == MG_OUT_BOUND) {
        CHECK(c.bound && p.root == &g_bound[0] && p.rb == &g_bound[1] && p.dof == &g_bound[2], "the bound outputs");
        for (int k = 0; k < MG_PART_N; ++k) write_bound(w, k, part_device(w, k));
    } else if (p.out == MG_OUT_STAGE) {
        CHECK(p.root == g_stage && w.cid == 0, "the host stage is written eagerly, where the last fetch staged");
        for (int k = 0; k < MG_PART_N; ++k) w.hs[k] = part_device(w, k);
    }
    w.F.end_simulate(p, w.cid);
    CHECK(!w.F.step(w.cid, false).root_src && !w.F.step(w.cid, false).tgt[0], "a set still pending after its simulate");
}

static void apply(World& w, const Cfg& c, Trace& t, int call) {
    t.call[t.n++] = call;
    float* src = &g_src[w.n];
    const uint32_t v = 100u + 37u * (uint32_t)w.n + (uint32_t)call;   // what this call's source holds
    w.srcv[w.n] = v;
    w.made[w.n] = (uint8_t)w.cid;
    ++w.n;
    switch (call) {
        case ROOT_DEV: case ROOT_DEV_IDX: case ROOT_HOST: {
            const bool host = call == ROOT_HOST, idx = call == ROOT_DEV_IDX;
            w.tR = idx ? mix(w.tR, v, 5) : v;
            const MgFusion::Set f = w.F.set_root(src, host, idx, c.roots_free, w.cid);
            w.set_how = f.how;
            set_checks(w, c, t, f, host && !idx);
            scatter_root(w, t, f.first);
            if (f.how == MG_SET_NOW) w.mR = idx ? mix(w.mR, v, 5) : v;
            if (f.how == MG_SET_DEFER_MAPPED) {   // copied at the call
                w.srcv[kMaxLen] = v;
                w.made[kMaxLen] = 0;
                w.F.root_mapped(kMapped);
            }
            break;
        }
        case RB_SET:
            w.tR = mix(w.tR, v, 6); w.tB = mix(w.tB, v, 6);
            scatter_root(w, t, w.F.set_rigid_body(w.cid));
            CHECK(w.F.last_set_deferred == 0, "mg_last_set_deferred after a rigid-body set");
            w.mR = mix(w.mR, v, 6); w.mB = mix(w.mB, v, 6);
            break;
        case DOF_SET:
            w.tD = mix(w.tD, v, 8);
            w.F.set_dof_state();
            CHECK(w.F.last_set_deferred == 0, "mg_last_set_deferred after a DOF-state set");
            w.mD = mix(w.mD, v, 8);
            break;
        case TGT_DEV: case TGT_DEV_IDX: {
            const bool idx = call == TGT_DEV_IDX;
            w.tT = idx ? mix(w.tT, v, 9) : v;
            const MgFusion::Set f = w.F.set_target(0, src, false, idx, w.cid);
            w.set_how = f.how;
            set_checks(w, c, t, f, false);
            copy_tgt(w, t, f.first);
            if (f.how == MG_SET_NOW) w.mT = idx ? mix(w.mT, v, 9) : v;
            break;
        }
        case SIMULATE: simulate(w, c, t); break;
        case REF_ROOT_BOUND: case REF_RB_BOUND: case REF_DOF_BOUND: refresh(w, c, t, call - REF_ROOT_BOUND, true); break;
        case REF_ROOT_OTHER: case REF_RB_OTHER: case REF_DOF_OTHER: refresh(w, c, t, call - REF_ROOT_OTHER, false); break;
        case FETCH: {
            if (w.cid != 0) break;   // refused while capturing
            scatter_root(w, t, w.F.read_state(w.cid));
            const int need = w.F.fetch(g_stage);
            w.fetch_need = need;
            for (int k = 0; k < MG_PART_N; ++k) {
                if ((need >> k) & 1) w.hs[k] = part_device(w, k);
                CHECK(w.hs[k] == part_truth(w, k), "1: a fetched part does not hold the state");
            }
            break;
        }
        case DISCARD: {
            // the truth forgets what is dropped: the sets still waiting, with the
            // earlier full sets they had replaced; the device never saw either
            const MgFusion::Step p = w.F.step(w.cid, false);
            if (p.root_src) w.tR = w.mR;
            if (p.tgt[0]) w.tT = w.mT;
            w.F.discard();
            break;
        }
        case REBIND: rebind(w, c); break;
        case CAPTURE_BEGINS: w.cid = ++w.ncap; break;
        case CAPTURE_ENDS: w.cid = 0; break;
    }
}

static void enumerate(const World& w, const Cfg& c, Trace& t, int depth) {
    for (int call = 0; call < N_CALLS; ++call) {
        World next = w;
        apply(next, c, t, call);
        if (depth + 1 < kLen) enumerate(next, c, t, depth + 1);
        --t.n;
    }
}

// ---- the sequences include/migym.h documents
static World run(const Cfg& c, Trace& t, World w, std::initializer_list<int> calls) {
    for (int call : calls) apply(w, c, t, call);
    return w;
}
static void documented() {
    {   // MG_FUSE_ALL, eager, per step: both sets deferred, every refresh after the simulate served by it
        const Cfg c{MG_FUSE_ROOT_SET | MG_FUSE_REFRESH | MG_FUSE_DOF_TARGETS | MG_FUSE_IN_CAPTURE | MG_FUSE_STEP_OUT, true, true, true};
        Trace t{&c, {}, 0};
        World w = make_world(c);
        for (int step = 0; step < 3; ++step) {
            w = run(c, t, w, {ROOT_DEV});
            CHECK(w.set_how == MG_SET_DEFER, "fused step: the root set is deferred");
            w = run(c, t, w, {TGT_DEV});
            CHECK(w.set_how == MG_SET_DEFER, "fused step: the target set is deferred");
            w = run(c, t, w, {SIMULATE});
            CHECK(w.sim_read_root && w.sim_read_tgt && w.sim_out == MG_OUT_BOUND, "fused step: the kernels read both sets and write the bound tensors");
            for (int call : {REF_ROOT_BOUND, REF_RB_BOUND, REF_DOF_BOUND}) {
                w = run(c, t, w, {call});
                CHECK(w.refresh_how == MG_REFRESH_SKIP, "fused step: a refresh after the simulate launches nothing");
            }
        }
    }
    {   // MG_FUSE_REFRESH alone: the root refresh is the paired gather, the rigid-body refresh is served by it
        const Cfg c{MG_FUSE_REFRESH, true, true, true};
        Trace t{&c, {}, 0};
        World w = make_world(c);
        for (int step = 0; step < 3; ++step) {
            w = run(c, t, w, {ROOT_DEV});
            CHECK(w.set_how == MG_SET_NOW, "refresh fusion alone: the root set is a scatter");
            w = run(c, t, w, {TGT_DEV});
            CHECK(w.set_how == MG_SET_NOW, "refresh fusion alone: the target set is a copy");
            w = run(c, t, w, {SIMULATE});
            CHECK(!w.sim_read_root && !w.sim_read_tgt && w.sim_out == MG_OUT_NONE, "refresh fusion alone: a plain step");
            w = run(c, t, w, {REF_ROOT_BOUND});
            CHECK(w.refresh_how == MG_REFRESH_PAIRED, "refresh fusion alone: the root refresh is the paired gather");
            w = run(c, t, w, {REF_RB_BOUND});
            CHECK(w.refresh_how == MG_REFRESH_SKIP, "refresh fusion alone: the rigid-body refresh is served by it");
            w = run(c, t, w, {REF_DOF_BOUND});
            CHECK(w.refresh_how == MG_REFRESH_GATHER, "refresh fusion alone: the DOF refresh gathers");
        }
    }
    for (int flags : {0, MG_FUSE_ROOT_SET | MG_FUSE_REFRESH | MG_FUSE_DOF_TARGETS | MG_FUSE_IN_CAPTURE | MG_FUSE_STEP_OUT}) {
        // the CPU pipeline (host tensors, nothing bound): the set goes through the mapped
        // buffer, and after the first fetch the step writes the stage itself
        const Cfg c{flags, false, true, true};
        Trace t{&c, {}, 0};
        World w = make_world(c);
        for (int step = 0; step < 3; ++step) {
            w = run(c, t, w, {ROOT_HOST});
            CHECK(w.set_how == MG_SET_DEFER_MAPPED, "CPU pipeline: the host root set goes through the mapped buffer");
            w = run(c, t, w, {SIMULATE});
            CHECK(w.sim_read_root, "CPU pipeline: the kernel reads the mapped buffer");
            CHECK(w.sim_out == (step == 0 ? MG_OUT_NONE : MG_OUT_STAGE), "CPU pipeline: the step writes the stage from the first fetch on");
            w = run(c, t, w, {FETCH});
            CHECK(w.fetch_need == (step == 0 ? 7 : 0), "CPU pipeline: only the first fetch gathers");
        }
    }
}

int main() {
    std::vector<Cfg> cfgs;
    for (int flags = 0; flags < 32; ++flags)
        for (int m = 0; m < 8; ++m) cfgs.push_back({flags, bool(m & 1), bool(m & 2), bool(m & 4)});
    static_assert((MG_FUSE_ROOT_SET | MG_FUSE_REFRESH | MG_FUSE_DOF_TARGETS | MG_FUSE_IN_CAPTURE | MG_FUSE_STEP_OUT) == 31, "five bits");
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < cfgs.size();) {
            Trace t{&cfgs[i], {}, 0};
            enumerate(make_world(cfgs[i]), cfgs[i], t, 0);
        }
    };
    unsigned nthreads = std::thread::hardware_concurrency();
    nthreads = nthreads < 1 ? 1 : nthreads > 16 ? 16 : nthreads;
    std::vector<std::thread> pool;
    for (unsigned i = 1; i < nthreads; ++i) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
    double nseq = 1;
    for (int i = 0; i < kLen; ++i) nseq *= N_CALLS;
    std::printf("%zu configurations x %.0f sequences of %d calls\n", cfgs.size(), nseq, kLen);
    documented();
    std::printf("%d failures\n", failures.load());
    return failures.load() ? 1 : 0;
}

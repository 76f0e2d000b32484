// mg_fusion.h — the ledger of step fusion (mg_set_fusion, MG_FUSE_*): which set
// sources wait to be read by the next simulate, and which tensors already hold
// the current state. Plain C++17 with no HIP header, so that a host program can
// include it alone (tests/fusion_ledger_check.cpp drives it through every short
// call sequence against Isaac Gym's contract).
//
// The C ABI (migym_capi.cpp) asks the ledger at each event, issues the launch
// or copy the answer names, and reports back what it issued. Two value types
// carry all of it:
//   * MgDeferred — a full device set whose source the next step kernel reads
//     instead of a scatter / copy launch: the source and the stream capture the
//     set was made in. Four of them: the root state and the three DOF target
//     columns. A host root set of the CPU pipeline is deferred the same way,
//     through the sim's mapped input buffer.
//   * MgCopy — "this destination holds generation g of the state, written in
//     capture c". Six of them: the bound root, rigid-body and DOF tensors
//     (mg_bind_refresh_targets, mg_bind_dof_refresh_target), written by the
//     step kernels (MG_FUSE_STEP_OUT) or by the paired gather
//     (MG_FUSE_REFRESH); and the three parts of the host stage
//     (mg_fetch_host_state), written by the step kernels of the CPU pipeline.
// Two generations count the changes: the body state (every root or rigid-body
// set, every simulate) and the DOF state (every DOF-state set, every simulate).
// A capture id is whatever the caller derives from its stream: 0 means eager.
//
// The rules, each written once below:
//   * fuse_here — work is deferred or skipped eagerly, and inside a capture
//     only with MG_FUSE_IN_CAPTURE: a set left pending at the end of a captured
//     region would never be applied by its replays.
//   * same capture — a deferred set is read only by a simulate of the capture
//     it was made in, and a copy serves only a refresh of the capture that
//     wrote it (take_foreign, holds): a graph never relies on work it did not
//     record. Anything else is applied as the ordinary launch first — and a
//     set made eagerly is never recorded into a graph (Apply::outside), whose
//     every replay would apply it again.
//   * every reader of the body state applies a pending root set first
//     (read_state: the one call every reader makes).
//   * with all flags off nothing is deferred or skipped: Isaac Gym copies at
//     the set call and refreshes exactly what is asked.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/migym.h"

struct MgDeferred {
    const float* src = nullptr;      // null: nothing pending
    unsigned long long cap = 0;
};
struct MgCopy {
    float* at = nullptr;
    long long gen = -1;              // -1: holds nothing
    unsigned long long cap = 0;
};

enum { MG_PART_ROOT, MG_PART_RB, MG_PART_DOF, MG_PART_N };   // mg_fetch_host_state's part bits 0..2
enum { MG_SET_NOW, MG_SET_DEFER, MG_SET_DEFER_MAPPED };
enum { MG_OUT_NONE, MG_OUT_BOUND, MG_OUT_STAGE };
enum { MG_REFRESH_GATHER, MG_REFRESH_PAIRED, MG_REFRESH_SKIP };

struct MgFusion {
    int flags = 0;                   // MG_FUSE_*
    int last_set_deferred = 0;       // mg_last_set_deferred
    long long state_gen = 0, dof_gen = 0;
    MgDeferred root, tgt[3];         // tgt: position, velocity, force column
    MgCopy bound[MG_PART_N], stage[MG_PART_N];
    float* stage_at = nullptr;       // the stage the last fetch used: the step writes there

    int set_flags(int f) {
        const int prev = flags;
        flags = f & (MG_FUSE_ROOT_SET | MG_FUSE_REFRESH | MG_FUSE_DOF_TARGETS | MG_FUSE_IN_CAPTURE | MG_FUSE_STEP_OUT);
        return prev;
    }
    bool fuse_here(unsigned long long cid) const { return cid == 0 || (flags & MG_FUSE_IN_CAPTURE); }
    long long gen_of(int part) const { return part == MG_PART_DOF ? dof_gen : state_gen; }
    bool holds(const MgCopy& c, int part, const float* at, unsigned long long cid) const {
        return at && c.at == at && c.gen == gen_of(part) && c.cap == cid;
    }
    // A deferred set handed back to be applied as the ordinary launch (src null:
    // none); it is no longer pending. `outside`: it was made eagerly and is handed
    // back inside a capture: it lands once, on the stream it was made on, not as
    // a node of the graph, whose every replay would apply it again.
    struct Apply {
        const float* src;
        bool outside;
    };
    static Apply take(MgDeferred& d, unsigned long long cid) {
        const Apply a{d.src, d.src && d.cap == 0 && cid != 0};
        d.src = nullptr;
        return a;
    }
    static Apply take_foreign(MgDeferred& d, unsigned long long cid) {
        return d.src && d.cap != cid ? take(d, cid) : Apply{nullptr, false};
    }

    // ---- sets. `first`: a pending set to apply before anything else.
    struct Set {
        int how;
        Apply first;
    };
    // MG_SET_DEFER: src waits for the next simulate's free-body kernel (a later
    // full set replaces it). MG_SET_DEFER_MAPPED (a full host set, eager): the
    // caller copies src into its mapped buffer and reports it (root_mapped).
    Set set_root(const float* src, bool src_host, bool indexed, bool roots_free, unsigned long long cid) {
        ++state_gen;
        last_set_deferred = 0;
        const bool full = !indexed && roots_free;
        if (full && !src_host && (flags & MG_FUSE_ROOT_SET) && fuse_here(cid)) {
            const Set r{MG_SET_DEFER, take_foreign(root, cid)};
            root = {src, cid};
            last_set_deferred = 1;
            return r;
        }
        if (full && src_host && cid == 0) {
            root.src = nullptr;
            return {MG_SET_DEFER_MAPPED, {nullptr, false}};
        }
        return {MG_SET_NOW, take(root, cid)};
    }
    void root_mapped(const float* mapped) { root = {mapped, 0}; }
    Apply set_rigid_body(unsigned long long cid) {   // a reader too: returns read_state()
        ++state_gen;
        last_set_deferred = 0;
        return take(root, cid);
    }
    void set_dof_state() {
        ++dof_gen;
        last_set_deferred = 0;
    }
    Set set_target(int k, const float* src, bool src_host, bool indexed, unsigned long long cid) {
        last_set_deferred = 0;
        if (!src_host && !indexed && (flags & MG_FUSE_DOF_TARGETS) && fuse_here(cid)) {
            const Set r{MG_SET_DEFER, take_foreign(tgt[k], cid)};
            tgt[k] = {src, cid};
            last_set_deferred = 1;
            return r;
        }
        return {MG_SET_NOW, take(tgt[k], cid)};
    }
    void discard() {
        root.src = nullptr;
        for (MgDeferred& t : tgt) t.src = nullptr;
    }

    // a reader of the body state: the pending root set to scatter first
    Apply read_state(unsigned long long cid) { return take(root, cid); }
    bool root_pending() const { return root.src != nullptr; }

    // ---- simulate. begin: the deferred sets this simulate's kernels will not
    // read (made in another capture, or no kernel of this model reads them), to
    // apply as ordinary launches first.
    struct Begin {
        Apply root, tgt[3];
    };
    Begin begin_simulate(unsigned long long cid, bool reads_root, bool reads_tgt) {
        Begin b{reads_root ? take_foreign(root, cid) : take(root, cid), {}};
        for (int k = 0; k < 3; ++k) b.tgt[k] = reads_tgt ? take_foreign(tgt[k], cid) : take(tgt[k], cid);
        return b;
    }
    // what the step kernels read in place of the sim's own state and targets
    // (null: nothing), and where they write the refreshed rows themselves: the
    // bound tensors (each optional), else the host stage (`root`: its base)
    struct Step {
        const float* root_src;
        const float* tgt[3];
        int out;
        float *root, *rb, *dof;
    };
    Step step(unsigned long long cid, bool writes_rows) const {
        Step p{root.src, {tgt[0].src, tgt[1].src, tgt[2].src}, MG_OUT_NONE, nullptr, nullptr, nullptr};
        const MgCopy* b = bound;
        if (writes_rows && (flags & MG_FUSE_STEP_OUT) && fuse_here(cid) && (b[0].at || b[1].at || b[2].at)) {
            p.out = MG_OUT_BOUND;
            p.root = b[MG_PART_ROOT].at; p.rb = b[MG_PART_RB].at; p.dof = b[MG_PART_DOF].at;
        } else if (writes_rows && stage_at && cid == 0) {
            p.out = MG_OUT_STAGE;
            p.root = stage_at;
        }
        return p;
    }
    // the launches of `p` were issued: its sets are consumed, its outputs hold the new state
    void end_simulate(const Step& p, unsigned long long cid) {
        discard();
        ++state_gen;
        ++dof_gen;
        for (int k = 0; k < MG_PART_N; ++k) {
            if (p.out == MG_OUT_BOUND && bound[k].at) bound[k] = {bound[k].at, gen_of(k), cid};
            if (p.out == MG_OUT_STAGE) stage[k] = {stage_at, gen_of(k), 0};
        }
    }

    // ---- refresh of part `part` into dst. MG_REFRESH_SKIP: dst is the bound
    // tensor and holds the state; MG_REFRESH_PAIRED: the bound root and
    // rigid-body tensors in one gather. The caller reports the gather it issued.
    struct Refresh {
        int how;
        bool stamps_rb;
        float* rb;   // MG_REFRESH_PAIRED: the bound rigid-body tensor
    };
    Refresh refresh(int part, const float* dst, bool dst_host, unsigned long long cid, bool has_actors) const {
        const float* at = dst_host ? nullptr : dst;
        const bool is_bound = at && at == bound[part].at;
        const int served = part == MG_PART_RB ? MG_FUSE_REFRESH | MG_FUSE_STEP_OUT : MG_FUSE_STEP_OUT;
        if ((flags & served) && fuse_here(cid) && holds(bound[part], part, at, cid)) return {MG_REFRESH_SKIP, false, nullptr};
        if (part == MG_PART_ROOT && is_bound && bound[MG_PART_RB].at && (flags & MG_FUSE_REFRESH) && fuse_here(cid) &&
            has_actors)
            return {MG_REFRESH_PAIRED, true, bound[MG_PART_RB].at};
        return {MG_REFRESH_GATHER, part == MG_PART_RB && is_bound, nullptr};
    }
    void refreshed(const Refresh& r, unsigned long long cid) {
        if (r.stamps_rb) bound[MG_PART_RB] = {bound[MG_PART_RB].at, state_gen, cid};
    }
    // rebinding forgets what the tensors held: the next refresh gathers
    void bind(float* root_dst, float* rb_dst) {
        bound[MG_PART_ROOT] = {root_dst, -1, 0};
        bound[MG_PART_RB] = {rb_dst, -1, 0};
    }
    void bind_dof(float* dof_dst) { bound[MG_PART_DOF] = {dof_dst, -1, 0}; }

    // ---- the host stage. fetch: the step kernels write into `base` from now
    // on; returns the part bits 0..2 that `base` does not hold and need a gather.
    int fetch(float* base) {
        stage_at = base;
        int need = 0;
        for (int k = 0; k < MG_PART_N; ++k)
            if (!holds(stage[k], k, base, 0)) need |= 1 << k;
        return need;
    }
    void stage_freed(const float* base) {   // `base` is about to be reallocated
        for (MgCopy& c : stage)
            if (c.at == base) c = {};
        if (stage_at == base) stage_at = nullptr;
    }
    void stage_replaced(float* fallback) {  // the mapped stage was replaced: the step writes into `fallback`
        for (MgCopy& c : stage) c = {};
        stage_at = fallback;
    }
};

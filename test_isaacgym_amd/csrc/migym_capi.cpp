// migym_capi.cpp — host side of libmigym.so: the C ABI declared in
// include/migym.h. Owns the engine state in HBM (SoA, env index as the
// coalesced axis), launches the step kernels and the tensor-API copy kernels on
// the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <string>
#include <map>
#include <vector>

#include "mg_internal.h"
#include "mg_chainlink.h"
#include "mg_attractor.h"
#include "mg_layout.h"
#include "mg_route.h"
#include "mg_fusion.h"

thread_local MgKernelTimer* mg_timer = nullptr;

namespace {

thread_local std::string g_err;
thread_local int g_err_code = MG_OK;   // of g_err (mg_last_error_code)

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    g_err_code = code;
    return code;
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(MG_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Owner of one allocation released by Free: move-only, frees on destruction or
// when assigned over, converts to T* where the raw pointer is used.
template <class T, hipError_t (*Free)(void*)>
struct Owned {
    T* p = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (p) (void)Free(p);
        p = nullptr;
    }
    operator T*() const { return p; }
};
// device memory; alloc() replaces what it held, with max(n, 1) elements
template <class T>
struct DevBuf : Owned<T, hipFree> {
    hipError_t alloc(size_t n) {
        this->reset();
        return hipMalloc((void**)&this->p, std::max<size_t>(n, 1) * sizeof(T));
    }
    hipError_t zero(size_t n) {    // alloc + clear
        hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemset(this->p, 0, std::max<size_t>(n, 1) * sizeof(T));
    }
    hipError_t upload(const T* h, size_t n, size_t room = 0) {   // alloc max(n, room) + copy n
        hipError_t e = alloc(std::max(n, room));
        return e != hipSuccess || n == 0 || !h ? e : hipMemcpy(this->p, h, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T>& h, size_t room = 0) { return upload(h.data(), h.size(), room); }
};
// page-locked host memory; mapped: for hipHostGetDevicePointer
template <class T>
struct HostBuf : Owned<T, hipHostFree> {
    hipError_t alloc(size_t n, bool mapped) {
        this->reset();
        return hipHostMalloc((void**)&this->p, n * sizeof(T),
                             mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault);
    }
};

// host AoS [n][ncol] -> device SoA [ncol][n]
template <class T>
std::vector<T> to_soa(const T* aos, int n, int ncol) {
    std::vector<T> soa((size_t)n * ncol);
    for (int i = 0; i < n; ++i)
        for (int f = 0; f < ncol; ++f) soa[(size_t)f * n + i] = aos[(size_t)i * ncol + f];
    return soa;
}

// what migym_capi.cpp adds to an articulation group of the layout plan (MgLayout::groups):
// k_artic_chain's shared constants (mg_chainlink.h): whether the stepped
// instances' DOF properties agree (upload and mg_set_dof_props), the
// constants themselves
struct ArticGroup {
    bool uni_dof = false;
    float uni[MG_CHAIN_UNI_N] = {};
};

static_assert(RS_G0 == MG_SENS_I_G0 && RS_LINK0 == MG_SENS_I_LINK0 && RS_LINK == MG_SENS_I_LINK && RS_MASK == MG_SENS_I_MASK &&
              RS_FLAGS == MG_SENS_I_FLAGS && RS_ART == MG_SENS_I_ART && RS_OUT == MG_SENS_I_OUT && RS_HIST == MG_SENS_I_HIST &&
              RS_OWNER == MG_SENS_I_OWNER && RS_I_N == MG_SENS_I_N && RS_F_N == MG_SENS_F_N && RS_ART_N == MG_SART_I_N,
              "mg_route.h packs the force sensor tables in mg_internal.h's columns");
static_assert(sizeof(MgSlotRec) == sizeof(std::array<int, 4>), "MgLayout::slot_rec is uploaded as MgSlotRec");
// the device headers' constants the planner needs
MgLayoutSizes layout_sizes() {
    return {MG_MAX_LINKS, MG_MAX_DOFS,
            MG_ENV_I_N, MG_ENV_MAXF, MG_ENV_MAXS, MG_ENV_SLOTS_WIDE, MG_ENV_FREE0, MG_ENV_STATIC0,
            MG_PILE_I_N, MG_PILE_MAXB, MG_PILE_ST0, MG_PILE_MAXPAIRS, MG_PILE_MAXSH, MG_PILE_GROUND,
            MG_TREC_N, MG_TREC_MASS, MG_OBB_N,
            mg_env_ctab_floats(), {mg_env_ctab_record_floats(0), mg_env_ctab_record_floats(1)}};
}

// The device buffers mg_upload_model fills from the layout plan, committed to
// the sim as one (mg_sim derives from it: s->d_state).
struct ModelBufs {
    DevBuf<float> d_state;     // [13][nb]
    DevBuf<float> d_mass;      // [12][nb]
    // Bodies are stored in an internal order (free bodies first, by launch group
    // and template; then each articulation's links contiguously; then the rest)
    // so every kernel's lanes touch contiguous SoA slots. Tensors stay in the
    // global (Isaac Gym) order: the gather / scatter index maps fold in `perm`.
    DevBuf<int> d_body_tmpl;   // [nb] internal order
    DevBuf<int> d_free_global; // [nf] global ids of the free bodies (internal 0..nf-1)
    DevBuf<int> d_perm;        // [nb] global body -> internal slot
    DevBuf<float> d_tbf;
    DevBuf<float> d_trec;      // [ntb][MG_TREC_N] compact template records (k_rigid_step1)
    DevBuf<int> d_tbi;
    DevBuf<float> d_shapes;
    DevBuf<float> d_hulls;     // convex hull records (MG_SHAPE_CONVEX)
    DevBuf<float> d_shape_obb; // [ns][MG_OBB_N] shape-frame boxes (coupled step's pair screen)
    DevBuf<int> d_actor_root;  // [na] internal slot of each actor's root body
    DevBuf<int> d_body_actor;  // [nb] global body -> the actor it is the root of, or -1
    DevBuf<int> d_root_row;    // [nb] internal slot -> actor row, -1 for non-roots (fused root sets)
    DevBuf<int> d_slot_global; // [nb] internal slot -> global body (rigid-body tensor row)
    DevBuf<int> d_slot_actor;  // [nb] internal slot -> actor row it is the root of, or -1
    DevBuf<MgSlotRec> d_slot_rec;   // [nb] {d_root_row, d_body_tmpl, d_slot_global, d_slot_actor} of each slot
    DevBuf<int> d_actor_dof;   // [na+1]
    DevBuf<float> d_cforce;    // [3][nb]
    DevBuf<float> d_ext;       // [6][nb]
    DevBuf<float> d_dof;       // [2][nd]: pos, vel
    DevBuf<float> d_dof_tgt;   // [3][nd]: target pos, target vel, actuation force
    DevBuf<float> d_dof_props; // [12][nd]
    DevBuf<float> d_dof_frc;   // [2][nd] DOF force tensor (mg_enable_dof_forces)
    DevBuf<int> d_artic;       // [nartic][4] sorted by template
    DevBuf<float> d_link_f;
    DevBuf<int> d_link_i;
    DevBuf<int> d_artic_step;  // [..][4] instances stepped by k_artic_chain / k_artic_lanes
    DevBuf<int> d_artic_split; // [step rows][MG_ARTIC_I_N] the owners' split rows (MgRoute::split)
    DevBuf<int> d_env;         // [n_coupled][MG_ENV_I_N] coupled envs, by group
    DevBuf<int> d_pairs;       // [..][4] candidate shape pairs of the coupled envs
    DevBuf<float> d_fpatch;    // [pairs][MG_FP_N] friction patch records (coupled step, persistent)
    DevBuf<float> d_gpatch;    // [MG_FP_N][nf1] ground patches of the single-shape free bodies (persistent)
    DevBuf<float> d_chain_uni; // [groups][MG_CHAIN_UNI_N] shared constants of chain groups (ArticGroup.uni)
    DevBuf<unsigned> d_fp_mask;   // [n_coupled][MG_FP_W] pairs holding a patch
    DevBuf<float> d_env_carry;    // [n_coupled][mg_env_carry_floats] coupled step state between substep launches
    DevBuf<float> d_env_ctab;     // [n_coupled][mg_env_ctab_floats] contacts of one substep (k_env_np -> k_env_step)
    // free-body piles (mg_pile.hip): coupled envs of more than MG_ENV_MAXF free
    // bodies and no articulation, one wavefront each
    DevBuf<int> d_pile_i;      // [n_pile][MG_PILE_I_N]
    DevBuf<int> d_pile_body;   // their free bodies' internal slots
    DevBuf<unsigned> d_pile_pairs;  // packed candidate pairs (local shape slots, mg_internal.h)
    DevBuf<int> d_pile_slots;  // [..][2] local shape slots: participant, shape
    // contact capacity report: the counters, and one flag word
    // per counted unit: the pile envs, then the coupled envs (rows of d_env),
    // then the multi-shape free bodies (slots nf1..nf_rigid-1)
    DevBuf<unsigned long long> d_cap;   // [MG_CAP_N]
    DevBuf<int> d_cap_flags;            // [n_pile + n_coupled + nf_rigid - nf1]
};

// the capacity report's counted units (ModelBufs::d_cap_flags): first unit of
// the coupled envs, of the multi-shape free bodies, and their total
inline int cap_env0(const MgLayout& L) { return L.n_pile; }
inline int cap_rigid0(const MgLayout& L) { return L.n_pile + L.n_coupled; }
inline int cap_units(const MgLayout& L) { return L.n_pile + L.n_coupled + (L.nf_rigid - L.nf1); }

// What mg_upload_model builds apart and commits to the sim as one: the plan
// (mg_layout.h: counts, storage order, index tables, groups and the host mirrors
// later calls read), its device buffers, what the groups carry besides, and the
// routing plan of the step features (mg_route.h) with the DOF
// property table it was planned from.
struct Model : ModelBufs {
    MgLayout layout;
    std::vector<ArticGroup> groups;   // by MgLayout::groups
    MgRoute route;
    std::vector<float> dof_props;     // [nd][MG_DOFPROP_N] as given
};
// the device form of the force sensor table (mg_set_force_sensors, MgSensorArgs)
struct SensBufs {
    DevBuf<int> d_sens_i;
    DevBuf<float> d_sens_f;
    DevBuf<int> d_sart_i;
    DevBuf<int> d_sens_flag;           // mark [n_sart], valid [n_sart], parity [1]
    DevBuf<float> d_sens_hist;
    DevBuf<float> d_sens_save;
    DevBuf<float> d_sens_out;          // [n_sens][6]
};
// the rigid contact list's staging and output (mg_set_contact_reporting)
struct CrepBufs {
    DevBuf<float> d_crep_cenv;         // [2 MG_ENV_MAXCT_WIDE][MG_CREP_N][n_coupled], column = row of d_env
    DevBuf<int> d_crep_cenv_n;         // [n_coupled]
    DevBuf<int> d_crep_col;            // [n_coupled] coupled env k -> its column
    DevBuf<float> d_crep_pile;         // [MG_PILE_MAXPT][MG_CREP_N][n_pile]
    DevBuf<int> d_crep_pile_n;         // [n_pile]
    DevBuf<float> d_crep_free;         // [MG_CREP_FREE_CAP][MG_CREP_N][nf_rigid]
    DevBuf<int> d_crep_free_n;         // [nf_rigid]
    DevBuf<int> d_crep_env;            // [owners] owner -> env
    DevBuf<int> d_crep_blk;            // [blocks] pass 1 -> pass 2
    DevBuf<mg_rigid_contact> d_crep_out;
    DevBuf<int> d_crep_hdr;            // [2]
};
// sleeping (mg_set_sleeping, mg_sleep.hip): the island tables of the layout plan
// and the pass's state, allocated while sleeping is on
struct SleepBufs {
    DevBuf<int> d_body0, d_body, d_dof0, d_dof;   // CSR island -> storage slots / DOFs
    DevBuf<int> d_body_island, d_actor_island;    // [nb] slot -> island, [na] actor -> island (-1: none)
    DevBuf<float> d_body_k;                       // [nb] 4 r_b^2
    DevBuf<int> d_timer, d_asleep;                // [islands]; timer -1: no anchor taken yet
    DevBuf<float> d_anchor;                       // [7][nb]
    DevBuf<float> d_dof_q;                        // [nd]
    DevBuf<int> d_idx;                            // mg_sleep_state's [na] device copy, the host wakes' island lists
    size_t idx_n = 0;
};

}  // namespace

struct mg_sim : Model, SensBufs, CrepBufs {
    int device = 0;
    mg_sim_params params{};
    bool uploaded = false;

    MgFusion fuse;    // step fusion (mg_set_fusion): the deferred sets and the fresh copies
    hipStream_t set_st[4] = {};   // the stream each deferred set was made on: root, target columns (apply_stream)
    bool ext_pending = false;

    DevBuf<float> d_stage;     // host-transfer staging (floats)
    size_t stage_n = 0;
    // CPU pipeline (host state tensors): a full host root set is read by the next
    // step kernel (no scatter launch; h_root_in below); and from the
    // first mg_fetch_host_state on, the step kernels that write their own rows
    // (step_out_ok) write root / rigid-body / DOF rows into d_host_out, laid out as
    // the host stage, so the fetch copies them without gathering
    // host sources are copied at the set call into this page-locked buffer (then
    // sent in stream order), so the caller may overwrite its tensor right away —
    // Isaac Gym's copy-at-set — even though the transfer itself is asynchronous;
    // pin_ev: the last transfer out of it (waited on before it is refilled)
    HostBuf<char> h_pin;
    size_t h_pin_n = 0;
    hipEvent_t pin_ev = nullptr;
    bool pin_ev_pending = false;
    DevBuf<float> d_host_out;
    size_t host_out_n = 0;
    // zero-copy variants (mg_host_stage): the host stage itself, page-locked and
    // mapped into the device's address space — the step kernels write their rows
    // into it over PCIe and the fetch's remaining gathers do too (no copy); and
    // a mapped input buffer the step kernel reads a host root set from
    // (root_ev: its last reader, waited on before it is refilled)
    bool has_light = false;           // mg_set_light (else the default light)
    mg_light light{};
    HostBuf<float> h_stage;
    float* d_stage_alias = nullptr;
    size_t h_stage_n = 0;
    HostBuf<float> h_root_in;
    float* d_root_in_alias = nullptr;
    hipEvent_t root_ev = nullptr;
    bool root_ev_pending = false;
    DevBuf<int> d_stage_idx;
    size_t stage_idx_n = 0;

    // camera render (mg_render.hip)
    DevBuf<float> d_rstate;    // [13][nb] pose snapshot of render_all_camera_sensors
    bool rstate_valid = false;
    DevBuf<MgRShape> d_rshapes;
    DevBuf<int> d_env_shape_first;
    int n_rshapes = 0;
    bool render_ready = false;
    DevBuf<MgRenderCam> d_cams;
    int cam_cap = 0;
    std::vector<mg_camera> cam_host;      // last uploaded table (as given)
    std::vector<MgRenderCam> cam_dev;     // its device form
    int cam_blocks = 0;
    hipEvent_t rev_b = nullptr, rev_e = nullptr;
    bool rendered = false;

    // Which launches the feature tables below imply, and what each carries, is
    // Model::route (mg_route.h): every call that changes a table plans it anew.

    // rigid-body attractors (mg_set_attractors, mg_attractor.h). The table as
    // given; its device form (MG_ATTR_N floats per record, built in the
    // page-locked h_attr and sent by the next simulate when attr_dirty) and
    // the internal slot -> record map
    std::vector<mg_attractor> attrs;
    DevBuf<float> d_attr;
    DevBuf<int> d_attr_idx;            // [nb]
    HostBuf<float> h_attr;
    hipEvent_t attr_ev = nullptr;
    bool attr_ev_pending = false, attr_dirty = false;

    // DOF force tensor (mg_enable_dof_forces): d_dof_frc holds the
    // step kernels' rows [nd], then the per-DOF reporting flags [nd] the refresh applies

    // force sensors (mg_set_force_sensors, mg_sensor.hip). The
    // table as given and its device form (SensBufs, from the route's host form),
    // allocated by the first table with a sensor
    std::vector<mg_force_sensor> sensors;
    DevBuf<float> d_ctorque;           // [3][nb], allocated with the first sensor table

    // rigid contact list (mg_set_contact_reporting, mg_contact.hip, DESIGN.md
    // §3.14). While route.crep the reporting builds of the step kernels fill the
    // staging records and k_contact_compact packs them into d_crep_out; the
    // buffers (CrepBufs) are allocated by the call that turns reporting on. crep_valid: a
    // reporting simulate has run since. The header (true total, stored total)
    // is kept on the device and in mapped host memory, which the refresh reads
    // after waiting for the stream.
    bool crep_valid = false;
    int crep_capacity = 0;
    HostBuf<int> h_crep_hdr;            // [2] mapped, page-locked
    int* d_crep_hdr_alias = nullptr;      // its device address

    // sleeping (mg_set_sleeping): off unless both figures are positive; the
    // buffers exist while it is on and a model is uploaded
    bool sleep_on = false;
    float sleep_threshold = 0.0f, sleep_window = 0.0f;
    SleepBufs sleep;

    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool timing = false;          // mg_set_kernel_timing: events around eager launches
    bool timed_step = false;      // the last simulate recorded ev_begin / ev_end
    hipStream_t last_stream = nullptr;
    bool stepped = false;
    bool capturing = false;       // the last simulate was recorded into a graph
    int cus = 256;                // the device's compute units (MgRun::cus), read once at mg_create_sim
    // the builds the last simulate launched, in launch order (mg_debug_step_builds, mg_last_rigid_form)
    std::vector<MgBuild> builds;
    // ring of per-simulate event pairs for live kernel timing (bench.py roofline)
    static constexpr int kRing = 256;
    static constexpr int kKern = 8;   // kernels timed per simulate (dispatch timestamps)
    hipEvent_t ring_b[kRing] = {}, ring_e[kRing] = {};
    hipEvent_t kern_b[kRing][kKern] = {}, kern_e[kRing][kKern] = {};
    int kern_n[kRing] = {};
    int kern_miss[kRing] = {};    // launches of that simulate past kKern (untimed)
    long long ring_n = 0;
};

namespace {

MgStep make_step(const mg_sim_params& p) {
    MgStep P{};
    const int ss = p.substeps > 0 ? p.substeps : 1;
    const int np = p.num_position_iterations > 0 ? p.num_position_iterations : 1;
    P.substeps = ss;
    P.npos = np;
    P.nvel = p.num_velocity_iterations > 0 ? p.num_velocity_iterations : 0;
    P.h = p.dt / (float)ss;
    P.sub = P.h / (float)np;
    P.inv_sub = 1.0f / P.sub;
    P.inv_h = 1.0f / P.h;
    P.inv_dt = 1.0f / p.dt;
    for (int k = 0; k < 3; ++k) P.g[k] = p.gravity[k];
    P.contact_offset = p.contact_offset;
    P.rest_offset = p.rest_offset;
    P.max_depen = p.max_depenetration_velocity;
    P.bounce_thresh = p.bounce_threshold_velocity;
    P.fric_offset = p.friction_offset_threshold;
    P.fric_corr = p.friction_correlation_distance;
    P.has_ground = p.has_ground;
    const float nx = p.ground_normal[0], ny = p.ground_normal[1], nz = p.ground_normal[2];
    P.n[0] = nx; P.n[1] = ny; P.n[2] = nz;
    P.pd = p.ground_distance;
    // tangent basis: t1 = normalize(n x a), t2 = n x t1
    float ax = 1.0f, ay = 0.0f, az = 0.0f;
    if (!(std::fabs(nx) < 0.9f)) { ax = 0.0f; ay = 1.0f; }
    float t1x = ny * az - nz * ay, t1y = nz * ax - nx * az, t1z = nx * ay - ny * ax;
    const float inv = 1.0f / std::sqrt(t1x * t1x + t1y * t1y + t1z * t1z);
    t1x = t1x * inv; t1y = t1y * inv; t1z = t1z * inv;
    P.t1[0] = t1x; P.t1[1] = t1y; P.t1[2] = t1z;
    P.t2[0] = ny * t1z - nz * t1y;
    P.t2[1] = nz * t1x - nx * t1z;
    P.t2[2] = nx * t1y - ny * t1x;
    P.mu_ground = p.ground_dynamic_friction;
    P.e_ground = p.ground_restitution;
    return P;
}

int ensure_stage(mg_sim* s, size_t nfloat, size_t nidx) {
    if (nfloat > s->stage_n) {
        s->stage_n = 0;
        HIP_TRY(s->d_stage.alloc(nfloat));
        s->stage_n = nfloat;
    }
    if (nidx > s->stage_idx_n) {
        s->stage_idx_n = 0;
        HIP_TRY(s->d_stage_idx.alloc(nidx));
        s->stage_idx_n = nidx;
    }
    return MG_OK;
}

// gather `n` rows of `ncol` SoA fields into dst (host or device)
int refresh_rows(mg_sim* s, const float* soa, int stride, int ncol, const int* ids, int n, float* dst,
                 int dst_host, hipStream_t st) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!dst && n > 0) return fail(MG_ERR_ARG, "null destination");
    HIP_TRY(hipSetDevice(s->device));
    if (n == 0) return MG_OK;
    if (!dst_host) {
        HIP_TRY(mg_launch_gather_rows(soa, stride, ncol, ids, n, dst, st));
        return MG_OK;
    }
    int rc = ensure_stage(s, (size_t)n * ncol, 0);
    if (rc) return rc;
    HIP_TRY(mg_launch_gather_rows(soa, stride, ncol, ids, n, s->d_stage, st));
    HIP_TRY(hipMemcpyAsync(dst, s->d_stage, (size_t)n * ncol * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MG_OK;
}

// copy host data into the sim's page-locked buffer now and send it to the device
// in stream order: n parts (src[k], bytes[k]) to dst[k]
int pin_h2d(mg_sim* s, int n, const void* const* src, const size_t* bytes, void* const* dst, hipStream_t st) {
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += (bytes[k] + 255) & ~(size_t)255;
    if (total > s->h_pin_n) {
        if (s->pin_ev_pending) HIP_TRY(hipEventSynchronize(s->pin_ev));
        s->h_pin_n = 0;
        HIP_TRY(s->h_pin.alloc(total, false));
        s->h_pin_n = total;
    }
    if (!s->pin_ev) HIP_TRY(hipEventCreateWithFlags(&s->pin_ev, hipEventDisableTiming));
    if (s->pin_ev_pending) HIP_TRY(hipEventSynchronize(s->pin_ev));   // the previous transfer left it
    size_t at = 0;
    for (int k = 0; k < n; ++k) {
        std::memcpy(s->h_pin + at, src[k], bytes[k]);
        HIP_TRY(hipMemcpyAsync(dst[k], s->h_pin + at, bytes[k], hipMemcpyHostToDevice, st));
        at += (bytes[k] + 255) & ~(size_t)255;
    }
    HIP_TRY(hipEventRecord(s->pin_ev, st));
    s->pin_ev_pending = true;
    return MG_OK;
}

// stage a host source (and optional index list) to the device
int stage_src(mg_sim* s, const float* src, int src_host, size_t nfloat, const int* idx, int n_idx,
              hipStream_t st, const float** dsrc, const int** didx) {
    *dsrc = src;
    *didx = idx;
    if (!src_host) return MG_OK;
    int rc = ensure_stage(s, nfloat, idx ? (size_t)n_idx : 0);
    if (rc) return rc;
    const void* srcs[2] = {src, idx};
    const size_t bytes[2] = {nfloat * sizeof(float), idx && n_idx > 0 ? (size_t)n_idx * sizeof(int) : 0};
    void* dsts[2] = {s->d_stage, s->d_stage_idx};
    if ((rc = pin_h2d(s, bytes[1] ? 2 : 1, srcs, bytes, dsts, st))) return rc;
    *dsrc = s->d_stage;
    if (idx && n_idx > 0) *didx = s->d_stage_idx;
    return MG_OK;
}

// id of the stream capture in progress on st + 1, or 0 when st is not capturing
unsigned long long capture_id(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(st, &cs, &id) != hipSuccess || cs != hipStreamCaptureStatusActive) return 0;
    return id + 1;
}

// `st` now reads the mapped root input buffer, if that is what `src` is
int root_in_read(mg_sim* s, const float* src, hipStream_t st) {
    if (!src || src != s->d_root_in_alias) return MG_OK;
    HIP_TRY(hipEventRecord(s->root_ev, st));
    s->root_ev_pending = true;
    return MG_OK;
}

// Where a deferred set the ledger hands back is launched: on the caller's
// stream; one made eagerly and handed back inside a capture (a.outside) on the
// stream it was made on (set_st: root, target columns), where it lands once, as
// it did at the set call without fusion. Recorded into the graph, every replay
// would apply it again. (Made on the capturing stream itself, it can only be recorded.)
hipStream_t apply_stream(const mg_sim* s, int which, const MgFusion::Apply& a, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!a.outside || hipStreamIsCapturing(s->set_st[which], &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
        return st;
    return s->set_st[which];
}

// apply a root-state set the ledger had deferred (null: none) as the ordinary scatter
int apply_root(mg_sim* s, const MgFusion::Apply& a, hipStream_t st) {
    if (!a.src) return MG_OK;
    st = apply_stream(s, 0, a, st);
    HIP_TRY(mg_launch_scatter_rows(a.src, MG_STATE_N, s->d_actor_root, nullptr, s->layout.na, s->layout.na, s->d_state, s->layout.nb, st));
    return root_in_read(s, a.src, st);
}
// what every reader of d_state opens with
int flush_root(mg_sim* s, hipStream_t st) {
    return s->fuse.root_pending() ? apply_root(s, s->fuse.read_state(capture_id(st)), st) : MG_OK;
}

// apply a deferred DOF target column (0 pos, 1 vel, 2 force; null: none) as a copy
int apply_tgt(mg_sim* s, int k, const MgFusion::Apply& a, hipStream_t st) {
    if (!a.src) return MG_OK;
    HIP_TRY(hipMemcpyAsync(s->d_dof_tgt + (size_t)k * s->layout.nd, a.src, (size_t)s->layout.nd * sizeof(float),
                           hipMemcpyDeviceToDevice, apply_stream(s, 1 + k, a, st)));
    return MG_OK;
}

// ---- sleeping ----
// the island tables and a fresh pass state (no island asleep, no anchor taken) for layout L
int sleep_alloc(const MgLayout& L, SleepBufs& B) {
    HIP_TRY(B.d_body0.upload(L.island_body0));
    HIP_TRY(B.d_body.upload(L.island_body));
    HIP_TRY(B.d_dof0.upload(L.island_dof0));
    HIP_TRY(B.d_dof.upload(L.island_dof));
    HIP_TRY(B.d_body_island.upload(L.body_island));
    HIP_TRY(B.d_actor_island.upload(L.actor_island));
    HIP_TRY(B.d_body_k.upload(L.body_k));
    HIP_TRY(B.d_timer.upload(std::vector<int>((size_t)L.n_island, -1)));
    HIP_TRY(B.d_asleep.zero((size_t)L.n_island));
    HIP_TRY(B.d_anchor.zero((size_t)7 * L.nb));
    HIP_TRY(B.d_dof_q.zero((size_t)L.nd));
    HIP_TRY(B.d_idx.alloc((size_t)std::max(L.na, 1)));
    B.idx_n = (size_t)std::max(L.na, 1);
    return MG_OK;
}
bool sleeping(const mg_sim* s) { return s->sleep_on && s->uploaded; }
// wake the islands of the actors didx[0..n) (device memory; null: every island), in stream order
int sleep_wake(mg_sim* s, const int* didx, int n, hipStream_t st) {
    if (!sleeping(s)) return MG_OK;
    const MgLayout& L = s->layout;
    if (!didx) HIP_TRY(mg_launch_wake(nullptr, L.n_island, nullptr, 0, L.n_island, s->sleep.d_timer, s->sleep.d_asleep, st));
    else HIP_TRY(mg_launch_wake(didx, n, s->sleep.d_actor_island, L.na, L.n_island, s->sleep.d_timer, s->sleep.d_asleep, st));
    return MG_OK;
}
// the wake of a call that has no stream (mg_set_dof_props, mg_set_sim_params, the attractor sets):
// islands `isl` (null: all), after the device's pending work and done when it returns
int sleep_wake_sync(mg_sim* s, const std::vector<int>* isl) {
    if (!sleeping(s) || (isl && isl->empty())) return MG_OK;
    const MgLayout& L = s->layout;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    if (isl) {
        if (isl->size() > s->sleep.idx_n) {
            s->sleep.idx_n = 0;
            HIP_TRY(s->sleep.d_idx.alloc(isl->size()));
            s->sleep.idx_n = isl->size();
        }
        HIP_TRY(hipMemcpy(s->sleep.d_idx, isl->data(), isl->size() * sizeof(int), hipMemcpyHostToDevice));
    }
    HIP_TRY(mg_launch_wake(isl ? (const int*)s->sleep.d_idx : nullptr, isl ? (int)isl->size() : L.n_island, nullptr, 0, L.n_island,
                           s->sleep.d_timer, s->sleep.d_asleep, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MG_OK;
}

int set_dof_columns(mg_sim* s, const float* src, int src_host, int ncol, float* dst0, float* dst1,
                    const int* idx, int n_idx, hipStream_t st) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (s->layout.nd == 0) return MG_OK;
    if (!src) return fail(MG_ERR_ARG, "null source tensor");
    if (idx && n_idx < 0) return fail(MG_ERR_ARG, "negative index count");
    HIP_TRY(hipSetDevice(s->device));
    const float* dsrc;
    const int* didx;
    int rc = stage_src(s, src, src_host, (size_t)s->layout.nd * ncol, idx, n_idx, st, &dsrc, &didx);
    if (rc) return rc;
    if ((rc = sleep_wake(s, idx ? didx : nullptr, n_idx, st))) return rc;   // autowake: the set actors' islands
    float* dst[2] = {dst0, dst1};
    if (idx)
        HIP_TRY(mg_launch_scatter_dofs(dsrc, ncol, s->d_actor_dof, didx, n_idx, s->layout.na, s->layout.max_actor_dofs, dst, st));
    else
        HIP_TRY(mg_launch_scatter_dofs(dsrc, ncol, nullptr, nullptr, s->layout.nd, 0, 1, dst, st));
    return MG_OK;
}

}  // namespace

extern "C" {

int32_t mg_abi_version(void) { return MG_ABI_VERSION; }
const char* mg_last_error(void) { return g_err.c_str(); }
int32_t mg_last_error_code(void) { return g_err_code; }

int32_t mg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

mg_sim* mg_create_sim(int32_t device, const mg_sim_params* params) {
    if (!params) { fail(MG_ERR_ARG, "null params"); return nullptr; }
    int n = mg_device_count();
    if (n <= 0) { fail(MG_ERR_DEVICE, "no HIP device available (libmigym needs an MI355X)"); return nullptr; }
    if (device < 0 || device >= n) { fail(MG_ERR_DEVICE, "device %d out of range (%d visible)", device, n); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail(MG_ERR_DEVICE, "hipSetDevice(%d) failed", device); return nullptr; }
    mg_sim* s = new mg_sim();
    s->device = device;
    s->params = *params;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) s->cus = cus;
    for (int k = 0; k < mg_sim::kRing; ++k) {
        bool ok = hipEventCreate(&s->ring_b[k]) == hipSuccess && hipEventCreate(&s->ring_e[k]) == hipSuccess;
        for (int j = 0; j < mg_sim::kKern && ok; ++j)
            ok = hipEventCreate(&s->kern_b[k][j]) == hipSuccess && hipEventCreate(&s->kern_e[k][j]) == hipSuccess;
        if (!ok) {
            fail(MG_ERR_DEVICE, "hipEventCreate failed");
            mg_destroy_sim(s);
            return nullptr;
        }
    }
    return s;
}

void mg_destroy_sim(mg_sim* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    // the buffers go with the sim below (DevBuf, HostBuf)
    for (int k = 0; k < mg_sim::kRing; ++k) {
        if (s->ring_b[k]) (void)hipEventDestroy(s->ring_b[k]);
        if (s->ring_e[k]) (void)hipEventDestroy(s->ring_e[k]);
        for (int j = 0; j < mg_sim::kKern; ++j) {
            if (s->kern_b[k][j]) (void)hipEventDestroy(s->kern_b[k][j]);
            if (s->kern_e[k][j]) (void)hipEventDestroy(s->kern_e[k][j]);
        }
    }
    if (s->rev_b) (void)hipEventDestroy(s->rev_b);
    if (s->rev_e) (void)hipEventDestroy(s->rev_e);
    if (s->pin_ev) (void)hipEventDestroy(s->pin_ev);
    if (s->root_ev) (void)hipEventDestroy(s->root_ev);
    if (s->attr_ev) (void)hipEventDestroy(s->attr_ev);
    delete s;
}

int32_t mg_set_sim_params(mg_sim* s, const mg_sim_params* p) {
    if (!s || !p) return fail(MG_ERR_ARG, "null argument");
    s->params = *p;
    return sleep_wake_sync(s, nullptr);
}

// k_artic_chain's shared constants (mg_chainlink.h). Link mass constants and
// the gravity flag of a group whose stepped instances agree on them
// (MgArticGroup::uni_mass), from the first one's global rows.
static void chain_uni_mass(const mg_model* m, const MgArticGroup& g, ArticGroup& c) {
    const int b0 = g.step_body0[0];
    const float grav = m->tmpl_body_f[(size_t)m->body_tmpl[b0] * MG_TBODY_F_N + 4];
    for (int l = 1; l < g.nl; ++l) {
        const float* r = m->body_mass + (size_t)(b0 + l) * MG_MASS_N;
        const ChainLink k = chain_link_make(r[11], v3(r[8], r[9], r[10]), r[1], r[2], r[3], q4(r[4], r[5], r[6], r[7]));
        float* u = c.uni + MG_CHAIN_UNI_LINK + 10 * (l - 1);
        u[0] = k.m;
        u[1] = k.com.x; u[2] = k.com.y; u[3] = k.com.z;
        for (int j = 0; j < 6; ++j) u[4 + j] = k.ib[j];
    }
    c.uni[MG_CHAIN_UNI_GRAV] = grav;
}
// DOF properties (global DOF order, MG_DOFPROP_N per DOF): fields 0..8 of each
// DOF of the chain, when every stepped instance has the same
static void chain_uni_dof(const float* props, const MgArticGroup& g, ArticGroup& c) {
    const int d0 = g.step_dof0[0];
    bool ok = true;
    for (size_t i = 1; i < g.step_dof0.size() && ok; ++i)
        for (int d = 0; d < g.ndof && ok; ++d)
            ok = std::memcmp(props + (size_t)(g.step_dof0[i] + d) * MG_DOFPROP_N, props + (size_t)(d0 + d) * MG_DOFPROP_N,
                             9 * sizeof(float)) == 0;
    c.uni_dof = ok;
    c.uni[MG_CHAIN_UNI_DOFOK] = ok ? 1.0f : 0.0f;   // read by the kernel (graph replays see changes)
    if (!ok) return;
    for (int d = 0; d < g.ndof; ++d)
        for (int j = 0; j < 9; ++j) c.uni[MG_CHAIN_UNI_DOF + 9 * d + j] = props[(size_t)(d0 + d) * MG_DOFPROP_N + j];
}
static hipError_t chain_uni_upload(Model* s) {
    if (!s->d_chain_uni) return hipSuccess;
    std::vector<float> u(s->groups.size() * MG_CHAIN_UNI_N, 0.0f);
    for (size_t i = 0; i < s->groups.size(); ++i)
        std::memcpy(&u[i * MG_CHAIN_UNI_N], s->groups[i].uni, MG_CHAIN_UNI_N * sizeof(float));
    return hipMemcpy(s->d_chain_uni, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice);
}

// ---- the routing plan of the step features (mg_route.h) ----
// The sim's current feature tables as the planner's inputs; a call replaces the one it changes.
static MgRouteIn route_in(const mg_sim* s) {
    MgRouteIn in;
    in.attrs = s->attrs.data(); in.n_attr = (int)s->attrs.size();
    in.sensors = s->sensors.data(); in.n_sens = (int)s->sensors.size();
    in.crep = s->route.crep;
    in.dof_props = s->dof_props.empty() ? nullptr : s->dof_props.data();
    in.dof_frc_n = s->route.dof_frc_n;
    in.sleep = s->sleep_on;
    return in;
}
static int plan_route(const MgLayout& L, const MgRouteIn& in, MgRoute& R) {
    std::string err;
    if (int rc_ = mg_plan_route(L, in, R, err)) return fail(rc_, "%s", err.c_str());
    return MG_OK;
}
// `what` decides which kernels a simulate launches: a graph captured before the
// call would replay the old launches
static int refuse_captured(const mg_sim* s, const char* what, const char* verb = "call") {
    if (!s->capturing) return MG_OK;
    return fail(MG_ERR_STATE, "%s after the step was captured into a graph (the replays keep the old launches); %s it before "
                "the capture, or after an eager simulate", what, verb);
}

// Plan, then commit: mg_plan_layout derives every table on
// the host; the device buffers are filled into a Model built apart, which
// becomes the sim's only when every HIP call has succeeded. A refused or
// failed upload leaves the sim as it was (and frees what it had allocated).
int32_t mg_upload_model(mg_sim* s, const mg_model* m) {
    if (!s || !m) return fail(MG_ERR_ARG, "null argument");
    if (s->uploaded) return fail(MG_ERR_STATE, "model already uploaded");
    Model M;
    MgLayout& L = M.layout;
    std::string err;
    if (int rc_ = mg_plan_layout(s->params, *m, layout_sizes(), L, err)) return fail(rc_, "%s", err.c_str());
    HIP_TRY(hipSetDevice(s->device));
    const int nb = L.nb, na = L.na, nd = L.nd;
    M.groups.resize(L.groups.size());
    for (size_t gi = 0; gi < L.groups.size(); ++gi)
        if (L.groups[gi].uni_mass) {
            chain_uni_mass(m, L.groups[gi], M.groups[gi]);
            chain_uni_dof(m->dof_props, L.groups[gi], M.groups[gi]);
        }
    // the step features' routing: no attractor, sensor or reporting yet; joint
    // friction as the DOF property table has it
    M.dof_props.assign(m->dof_props, m->dof_props + (size_t)nd * MG_DOFPROP_N);
    MgRouteIn rin;
    rin.dof_props = nd > 0 ? M.dof_props.data() : nullptr;
    rin.sleep = s->sleep_on;
    if (int rc_ = plan_route(L, rin, M.route)) return rc_;

    // bodies, templates, shapes
    HIP_TRY(M.d_state.upload(L.state0));
    HIP_TRY(M.d_mass.upload(L.mass0));
    HIP_TRY(M.d_body_tmpl.upload(L.tmpl_int));
    HIP_TRY(M.d_free_global.upload(L.order.data(), (size_t)L.nf));
    HIP_TRY(M.d_perm.upload(L.perm));
    HIP_TRY(M.d_tbf.upload(m->tmpl_body_f, (size_t)L.ntb * MG_TBODY_F_N));
    HIP_TRY(M.d_tbi.upload(m->tmpl_body_i, (size_t)L.ntb * MG_TBODY_I_N));
    HIP_TRY(M.d_trec.upload(L.trec));
    HIP_TRY(M.d_shapes.upload(m->shapes, (size_t)L.ns * MG_SHAPE_STRIDE));
    HIP_TRY(M.d_hulls.upload(m->hulls, (size_t)L.nhull_floats));
    HIP_TRY(M.d_shape_obb.upload(L.shape_obb));
    // actors and the per-slot index tables
    HIP_TRY(M.d_actor_root.upload(L.root_int));
    HIP_TRY(M.d_body_actor.upload(L.body_actor));
    HIP_TRY(M.d_root_row.upload(L.root_row));
    HIP_TRY(M.d_slot_global.upload(L.order));
    HIP_TRY(M.d_slot_actor.upload(L.slot_actor));
    HIP_TRY(M.d_slot_rec.upload(reinterpret_cast<const MgSlotRec*>(L.slot_rec.data()), (size_t)nb));
    HIP_TRY(M.d_actor_dof.upload(m->actor_dof, (size_t)na + 1));
    HIP_TRY(M.d_cforce.zero((size_t)nb * 3));
    HIP_TRY(M.d_ext.zero((size_t)nb * 6));
    // DOFs
    HIP_TRY(M.d_dof.upload(to_soa(m->dof_state0, nd, 2)));
    HIP_TRY(M.d_dof_tgt.zero((size_t)nd * 3));
    HIP_TRY(M.d_dof_props.upload(to_soa(m->dof_props, nd, MG_DOFPROP_N)));
    HIP_TRY(M.d_dof_frc.zero((size_t)nd * 2));
    // articulations
    HIP_TRY(M.d_chain_uni.alloc(std::max<size_t>(M.groups.size(), 1) * MG_CHAIN_UNI_N));
    HIP_TRY(chain_uni_upload(&M));
    if (!M.route.split.empty()) HIP_TRY(M.d_artic_split.upload(M.route.split));
    HIP_TRY(M.d_artic.upload(L.artic_sorted));
    HIP_TRY(M.d_artic_step.upload(L.artic_step));
    HIP_TRY(M.d_link_f.upload(m->tmpl_link_f, (size_t)L.ntl * MG_LINK_F_N));
    HIP_TRY(M.d_link_i.upload(m->tmpl_link_i, (size_t)L.ntl * MG_LINK_I_N));
    // coupled envs: rows, pairs, friction patches (none yet: every pair starts
    // without anchors), the step's per-env records between its launches
    HIP_TRY(M.d_env.upload(L.env_flat));
    HIP_TRY(M.d_pairs.upload(L.pairs));
    const size_t nc = (size_t)std::max(L.n_coupled, 1);
    HIP_TRY(M.d_fpatch.zero(std::max<size_t>(L.pairs.size() / 4, 1) * MG_FP_N));
    HIP_TRY(M.d_fp_mask.zero(nc * MG_FP_W));
    HIP_TRY(M.d_env_carry.alloc(nc * mg_env_carry_floats()));
    HIP_TRY(M.d_env_ctab.alloc(nc * mg_env_ctab_floats()));
    HIP_TRY(M.d_gpatch.zero((size_t)std::max(L.nf1, 1) * MG_FP_N));   // no ground patch yet
    if (L.n_pile > 0) {
        HIP_TRY(M.d_pile_i.upload(L.pile_rows));
        HIP_TRY(M.d_pile_body.upload(L.pile_body));
        HIP_TRY(M.d_pile_pairs.upload(L.pile_pairs));
        HIP_TRY(M.d_pile_slots.upload(L.pile_slots, 2));
    }
    HIP_TRY(M.d_cap.zero(MG_CAP_N));
    HIP_TRY(M.d_cap_flags.zero((size_t)cap_units(L)));
    SleepBufs SB;   // sleeping was turned on before the upload
    if (s->sleep_on)
        if (int rc_ = sleep_alloc(L, SB)) return rc_;
    HIP_TRY(hipDeviceSynchronize());
    // ---- commit (nothing below fails); the initial state went to the device
    std::vector<float>().swap(L.state0);
    std::vector<float>().swap(L.mass0);
    static_cast<Model&>(*s) = std::move(M);
    s->sleep = std::move(SB);
    s->uploaded = true;
    return MG_OK;
}

// the deferred DOF target columns as the kernels' inputs, with write-through
static void fused_targets(const mg_sim* s, const MgFusion::Step& fs, const float*& tp, const float*& tv, const float*& tf,
                          float*& wp, float*& wv, float*& wf) {
    const float** in[3] = {&tp, &tv, &tf};
    float** out[3] = {&wp, &wv, &wf};
    for (int k = 0; k < 3; ++k) {
        *out[k] = nullptr;
        if (fs.tgt[k]) {
            *in[k] = fs.tgt[k];
            *out[k] = s->d_dof_tgt + (size_t)k * s->layout.nd;
        }
    }
}

// the force sensor kernels' argument block (mg_sensor.hip)
static MgSensorArgs sensor_args(const mg_sim* s, const MgStep& P) {
    MgSensorArgs A{};
    const int n_sart = s->route.n_sart;
    A.n = s->route.n_sens; A.n_art = n_sart; A.nb = s->layout.nb; A.nd = s->layout.nd; A.nhb = s->route.sens_nhb;
    A.sens_i = s->d_sens_i; A.sens_f = s->d_sens_f; A.sart_i = s->d_sart_i;
    A.perm = s->d_perm; A.link_i = s->d_link_i;
    A.state = s->d_state; A.mass = s->d_mass; A.body_tmpl = s->d_body_tmpl; A.tbf = s->d_tbf;
    A.ext = s->d_ext; A.cforce = s->d_cforce; A.ctorque = s->d_ctorque; A.dof = s->d_dof;
    A.hist = s->d_sens_hist; A.save = s->d_sens_save;
    A.mark = s->d_sens_flag; A.valid = s->d_sens_flag + n_sart; A.parity = s->d_sens_flag + 2 * (size_t)n_sart;
    A.out = s->d_sens_out;
    for (int k = 0; k < 3; ++k) A.g[k] = P.g[k];
    A.inv_dt = P.inv_dt;
    return A;
}

// Where the step kernels write the refreshed rows themselves: the bound tensors
// (MG_FUSE_STEP_OUT) or the host stage (mg_fetch_host_state), each optional; all null: nowhere.
// With them the ledger's answer itself (fs): the deferred sets these kernels read.
struct StepOut {
    float *rb = nullptr, *root = nullptr, *dof = nullptr;
    const int *out_body = nullptr, *out_root_row = nullptr;   // internal slot -> global body / actor row (or -1)
    MgFusion::Step fs{};
};
static StepOut step_out(const mg_sim* s, const MgFusion::Step& fs) {
    StepOut O;
    O.fs = fs;
    if (fs.out == MG_OUT_NONE) return O;
    O.out_body = s->d_slot_global;
    O.out_root_row = s->d_slot_actor;
    O.root = fs.root; O.rb = fs.rb; O.dof = fs.dof;
    if (fs.out == MG_OUT_STAGE) {   // the host stage's layout (mg_fetch_host_state)
        O.rb = fs.root + (size_t)s->layout.na * MG_STATE_N;
        O.dof = s->layout.nd ? fs.root + (size_t)(s->layout.na + s->layout.nb) * MG_STATE_N : nullptr;
    }
    return O;
}

// The argument blocks of the route's launches (mg_route.h). A launch's feature pointers follow
// its build's form and nothing else: each optional member is set exactly when the build
// dereferences it (mg_forms.h mg_build_needs), which the launcher checks again.
// An articulation group's launch: over all its stepped instances, or, in a group with owners
// (l.split: rows loaded from the split table, not computed), over the plain ones, those that
// hold a friction DOF or those that own an attractor.
static MgArticArgs artic_args(mg_sim* s, const MgLaunch& l, const MgBuild& b, const StepOut& O) {
    const MgArticGroup& g = s->layout.groups[l.group];
    const unsigned need = mg_build_needs(b);
    MgArticArgs A{};
    // the DOF part's validity is a flag in the block (MG_CHAIN_UNI_DOFOK), not
    // a launch choice: a captured launch follows later set_dof_props
    A.uni = need & MG_NEED_UNI ? s->d_chain_uni + (size_t)l.group * MG_CHAIN_UNI_N : nullptr;
    A.na = l.count; A.nb = s->layout.nb; A.nd = s->layout.nd;
    A.artic_i = (l.split ? s->d_artic_split : s->d_artic_step) + (size_t)l.row0 * MG_ARTIC_I_N;
    A.aff = b.aff; A.ab0 = g.aff_b0; A.ad0 = g.aff_d0; A.ads = g.aff_ds;
    A.out_aff = b.out_aff; A.og0 = g.out_g0; A.or0 = g.out_r0;
    A.tmpl = g.tmpl; A.nl = g.nl; A.ndof = g.ndof; A.fixed_base = g.fixed_base; A.chain = g.chain; A.nbl = g.nbody;
    A.link_f = s->d_link_f + (size_t)g.first_link * MG_LINK_F_N;
    A.link_i = s->d_link_i + (size_t)g.first_link * MG_LINK_I_N;
    A.state = s->d_state; A.mass = s->d_mass; A.body_tmpl = s->d_body_tmpl; A.tbf = s->d_tbf;
    A.dof_pos = s->d_dof; A.dof_vel = s->d_dof + s->layout.nd;
    A.dof_tpos = s->d_dof_tgt; A.dof_tvel = s->d_dof_tgt + s->layout.nd; A.dof_force = s->d_dof_tgt + 2 * (size_t)s->layout.nd;
    fused_targets(s, O.fs, A.dof_tpos, A.dof_tvel, A.dof_force, A.tpos_w, A.tvel_w, A.force_w);
    A.dof_props = s->d_dof_props;
    A.ext = s->ext_pending ? s->d_ext : nullptr;
    A.cforce = s->d_cforce;
    A.dof_frc = need & MG_NEED_DOF_FRC ? s->d_dof_frc : nullptr;
    A.out_rb = O.rb; A.out_root = O.root; A.out_dof = O.dof;   // chain groups only (s->layout.step_out_ok)
    A.out_body = O.out_body; A.out_root_row = O.out_root_row;
    A.jfr = l.feat & RT_JFR ? 1 : 0;   // read by no kernel
    if (need & MG_NEED_ATTR) {
        A.attr_idx = s->d_attr_idx;
        A.attr = s->d_attr;
    }
    return A;
}

// the coupled step of one env group (mg_env.hip)
static MgEnvArgs env_args(mg_sim* s, const MgLaunch& l, const MgBuild& b, const MgFusion::Step& fs) {
    const MgEnvGroup& g = s->layout.env_groups[l.group];
    const unsigned need = mg_build_needs(b);
    MgEnvArgs A{};
    A.ne = g.count; A.nb = s->layout.nb; A.nd = s->layout.nd;
    A.env_i = s->d_env + (size_t)g.offset * MG_ENV_I_N;
    A.pairs = s->d_pairs;
    A.fpatch = s->d_fpatch;
    A.fp_mask = s->d_fp_mask + (size_t)g.offset * MG_FP_W;
    A.carry = s->d_env_carry + (size_t)g.offset * mg_env_carry_floats();
    A.ctab = s->d_env_ctab + (size_t)g.offset * mg_env_ctab_floats();
    A.nl = g.tmpl >= 0 ? g.nl : 0;
    A.ndof = g.tmpl >= 0 ? g.ndof : 0;
    A.floating = g.tmpl >= 0 ? g.floating : 0;
    A.max_free = g.max_free;
    A.link_f = s->d_link_f + (size_t)(g.tmpl >= 0 ? g.first_link : 0) * MG_LINK_F_N;
    A.link_i = s->d_link_i + (size_t)(g.tmpl >= 0 ? g.first_link : 0) * MG_LINK_I_N;
    A.state = s->d_state; A.mass = s->d_mass; A.body_tmpl = s->d_body_tmpl;
    A.tbf = s->d_tbf; A.tbi = s->d_tbi; A.shapes = s->d_shapes; A.hulls = s->d_hulls;
    A.shape_obb = s->d_shape_obb;
    A.nhull = s->layout.nhull_floats;
    A.nshape = s->layout.ns;
    A.dof_pos = s->d_dof; A.dof_vel = s->d_dof + s->layout.nd;
    A.dof_tpos = s->d_dof_tgt; A.dof_tvel = s->d_dof_tgt + s->layout.nd; A.dof_force = s->d_dof_tgt + 2 * (size_t)s->layout.nd;
    fused_targets(s, fs, A.dof_tpos, A.dof_tvel, A.dof_force, A.tpos_w, A.tvel_w, A.force_w);
    A.dof_props = s->d_dof_props;
    A.ext = s->ext_pending ? s->d_ext : nullptr;
    A.cforce = s->d_cforce;
    A.jfr = l.feat & RT_JFR ? 1 : 0;   // read by no kernel
    if (need & MG_NEED_ATTR) {
        A.attr_idx = s->d_attr_idx;
        A.attr = s->d_attr;
    }
    if (need & MG_NEED_CREP) {   // the reporting builds
        A.crep = s->d_crep_cenv + g.offset;
        A.crep_n = s->d_crep_cenv_n + g.offset;
        A.crep_body = s->d_slot_global;
        A.crep_stride = std::max(s->layout.n_coupled, 1);
    }
    if (need & MG_NEED_CTORQUE) A.ctorque = s->d_ctorque;   // the contact-moment builds
    A.dof_frc = need & MG_NEED_DOF_FRC ? s->d_dof_frc : nullptr;
    A.cap = {s->d_cap, s->d_cap_flags + cap_env0(s->layout) + g.offset};
    return A;
}

static MgPileArgs pile_args(const mg_sim* s, const MgBuild& b) {
    MgPileArgs A{};
    A.ne = s->layout.n_pile; A.nb = s->layout.nb;
    A.pile_i = s->d_pile_i; A.pile_body = s->d_pile_body; A.pairs = s->d_pile_pairs; A.slots = s->d_pile_slots;
    A.state = s->d_state; A.mass = s->d_mass; A.body_tmpl = s->d_body_tmpl; A.tbf = s->d_tbf;
    A.shapes = s->d_shapes; A.hulls = s->d_hulls; A.shape_obb = s->d_shape_obb;
    A.ext = s->ext_pending ? s->d_ext : nullptr;
    A.cforce = s->d_cforce;
    if (mg_build_needs(b) & MG_NEED_CREP) {   // the reporting build
        A.crep = s->d_crep_pile;
        A.crep_n = s->d_crep_pile_n;
        A.crep_body = s->d_slot_global;
    }
    A.cap = {s->d_cap, s->d_cap_flags};
    return A;
}

// the free-body step; a deferred root set (O.fs.root_src) is read by the kernel
static MgRigidArgs rigid_args(const mg_sim* s, const MgBuilds& b, const StepOut& O) {
    const unsigned need = mg_build_needs(b.one) | mg_build_needs(b.multi);
    MgRigidArgs A{};
    A.nf = s->layout.nf_rigid; A.nf1 = s->layout.nf1; A.nb = s->layout.nb; A.free_ids = nullptr;   // internal slots 0..nf-1
    A.state = s->d_state; A.mass = s->d_mass; A.body_tmpl = s->d_body_tmpl;
    A.tbf = s->d_tbf; A.tbi = s->d_tbi; A.shapes = s->d_shapes; A.hulls = s->d_hulls;
    A.trec = s->d_trec; A.ntb = s->layout.ntb;
    A.slot_rec = need & MG_NEED_SLOT_REC ? (const MgSlotRec*)s->d_slot_rec : nullptr;
    A.box_only = s->layout.free_flags.empty() ? 0 : s->layout.free_flags[0];
    A.gpatch = s->d_gpatch;
    A.gstride = std::max(s->layout.nf1, 1);
    A.ext = s->ext_pending ? s->d_ext : nullptr;
    A.cforce = s->d_cforce;
    if (need & MG_NEED_ATTR) {
        A.attr_idx = s->d_attr_idx;
        A.attr = s->d_attr;
    }
    if (need & MG_NEED_CREP) {   // the reporting builds
        A.crep = s->d_crep_free;
        A.crep_n = s->d_crep_free_n;
        A.crep_body = s->d_slot_global;
        A.crep_stride = std::max(s->layout.nf_rigid, 1);
    }
    if (O.fs.root_src) {
        A.root_src = O.fs.root_src;
        A.root_row = s->d_root_row;
    }
    A.out_rb = O.rb; A.out_root = O.root;
    A.out_body = O.out_body; A.out_root_row = O.out_root_row;
    A.cap = {s->d_cap, s->d_cap_flags + cap_rigid0(s->layout)};
    return A;
}

// the contact list of a frame: the staging records packed in owner order
static MgContactArgs contact_args(const mg_sim* s) {
    const int n[MG_CREP_FAMILIES] = {s->layout.nf_rigid, s->layout.n_coupled, s->layout.n_pile};
    const int cap[MG_CREP_FAMILIES] = {MG_CREP_FREE_CAP, 2 * MG_ENV_MAXCT_WIDE, MG_PILE_MAXPT};
    const float* stage[MG_CREP_FAMILIES] = {s->d_crep_free, s->d_crep_cenv, s->d_crep_pile};
    const int* count[MG_CREP_FAMILIES] = {s->d_crep_free_n, s->d_crep_cenv_n, s->d_crep_pile_n};
    MgContactArgs C{};
    for (int k = 0; k < MG_CREP_FAMILIES; ++k) {
        C.fam[k] = {n[k], cap[k], std::max(n[k], 1), stage[k], count[k], s->d_crep_env + C.n_own, nullptr};
        C.n_own += n[k];
    }
    C.fam[1].col = s->d_crep_col;
    C.nblk = (C.n_own + MG_CREP_BLOCK - 1) / MG_CREP_BLOCK;
    C.blk_sum = s->d_crep_blk;
    C.out = s->d_crep_out;
    C.capacity = s->crep_capacity;
    C.header = s->d_crep_hdr;
    C.header_host = s->d_crep_hdr_alias;
    return C;
}

int32_t mg_simulate(mg_sim* s, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "simulate before the model was uploaded");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const MgStep P = make_step(s->params);
    s->builds.clear();   // this simulate's (mg_debug_step_builds, mg_last_rigid_form)
    // Under HIP stream capture (a hipGraph of the tensor-API step) the launches
    // are recorded as graph nodes; the timing events are left out (they would
    // become fixed nodes of the graph) and fetch_results does not block.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cap));
    s->capturing = cap != hipStreamCaptureStatusNone;
    // ---- refusals. Rigid-body attractors, sensors, joint friction: a table
    // this build cannot honour is refused, never ignored
    const MgRoute& R = s->route;
    if (R.refusal) return fail(R.refusal, "%s", R.refusal_msg.c_str());
    if (s->attr_dirty && s->capturing)
        return fail(MG_ERR_STATE, "attractor table changed while the stream is being captured");
    // ---- begin: deferred sets this step's kernels do not read are applied as ordinary launches
    const unsigned long long cid = capture_id(st);
    const MgFusion::Begin fb =
        s->fuse.begin_simulate(cid, s->layout.nf_rigid > 0, !s->layout.groups.empty() || !s->layout.env_groups.empty());
    if (int rc_ = apply_root(s, fb.root, st)) return rc_;
    for (int k = 0; k < 3; ++k)
        if (int rc_ = apply_tgt(s, k, fb.tgt[k], st)) return rc_;
    MgKernelTimer timer{};
    struct TimerScope {
        ~TimerScope() { mg_timer = nullptr; }
    } timer_scope;
    int slot = 0;
    if (s->attr_dirty) {   // a changed attractor table is sent here, in stream order before the step
        HIP_TRY(hipMemcpyAsync(s->d_attr, s->h_attr, s->attrs.size() * MG_ATTR_N * sizeof(float),
                               hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(s->attr_ev, st));
        s->attr_ev_pending = true;
        s->attr_dirty = false;
    }
    const bool timed = s->timing && !s->capturing;
    if (timed) {
        slot = (int)(s->ring_n % mg_sim::kRing);
        s->ev_begin = s->ring_b[slot];
        s->ev_end = s->ring_e[slot];
        HIP_TRY(hipEventRecord(s->ev_begin, st));
        timer.start = s->kern_b[slot];
        timer.stop = s->kern_e[slot];
        timer.cap = mg_sim::kKern;
        mg_timer = &timer;
    }
    if (R.n_sens > 0) {
        // force sensors: which articulations begin the frame with a state set
        // (a deferred root set is applied first, so that the comparison sees it)
        if (int rc_ = flush_root(s, st)) return rc_;
        HIP_TRY(mg_launch_sensor_mark(sensor_args(s, P), st));
    }
    // ---- the launches. The kernels read the deferred sets of this capture, and
    // write the refreshed rows themselves where the ledger says: into the bound
    // tensors (MG_FUSE_STEP_OUT), else into the CPU pipeline's output stage
    // (mg_fetch_host_state: the library's own buffer, so no caller-visible tensor changes)
    const MgFusion::Step fs = s->fuse.step(cid, R.step_writes_rows);
    const StepOut O = step_out(s, fs);
    const MgRun run{mg_step_is_upz(P.n, P.t1, P.t2), s->ext_pending, O.rb || O.root, s->cus};
    for (const MgLaunch& l : R.launches) {
        // which kernel at which form: the chooser's answer (mg_route.h), recorded as launched
        const MgBuilds B = mg_route_builds(s->layout, l, run);
        if (B.one.kernel) s->builds.push_back(B.one);
        if (B.multi.kernel) s->builds.push_back(B.multi);
        hipError_t e = hipSuccess;
        switch (l.family) {
            case MG_FAM_ARTIC:
                e = B.one.kernel == MG_K_ARTIC_LANES ? mg_launch_artic_lanes(P, artic_args(s, l, B.one, O), B.one, st)
                                                     : mg_launch_artic_chain(P, artic_args(s, l, B.one, O), B.one, st);
                if (e != hipSuccess)
                    return fail(MG_ERR_DEVICE, "articulation step launch%s: %s",
                                l.feat & RT_JFR ? " (joint friction)" : l.feat & RT_ATTR ? " (attractors)" : "", hipGetErrorString(e));
                break;
            case MG_FAM_ENV:
                e = mg_launch_env_step(P, env_args(s, l, B.one, fs), B.one, st);
                if (e != hipSuccess) return fail(MG_ERR_DEVICE, "coupled env step launch: %s", hipGetErrorString(e));
                break;
            case MG_FAM_PILE:
                e = mg_launch_pile_step(P, pile_args(s, B.one), B.one, st);
                if (e != hipSuccess) return fail(MG_ERR_DEVICE, "pile step launch: %s", hipGetErrorString(e));
                break;
            default:
                HIP_TRY(mg_launch_rigid_step(P, rigid_args(s, B, O), B, st));
                if (int rc_ = root_in_read(s, fs.root_src, st)) return rc_;
        }
    }
    // ---- end: the deferred sets were read (and the targets written through), the outputs written
    s->fuse.end_simulate(fs, cid);
    // ---- sleeping: the pass over the islands, one launch per size class present
    if (sleeping(s)) {
        const MgLayout& L = s->layout;
        const double window = s->sleep_window, tol = window * std::sqrt(2.0 * (double)s->sleep_threshold);
        MgSleepArgs A{};
        A.nb = L.nb; A.nd = L.nd;
        A.window = (int)std::max(1l, std::lround(window / (double)s->params.dt));
        A.tol2 = (float)(tol * tol);
        A.body0 = s->sleep.d_body0; A.body = s->sleep.d_body; A.dof0 = s->sleep.d_dof0; A.dof = s->sleep.d_dof;
        A.body_k = s->sleep.d_body_k;
        A.state = s->d_state; A.dofs = s->d_dof;
        A.timer = s->sleep.d_timer; A.asleep = s->sleep.d_asleep; A.anchor = s->sleep.d_anchor; A.dof_q = s->sleep.d_dof_q;
        const int lanes[3] = {1, 16, 64};
        for (int c = 0; c < 3; ++c) {
            A.i0 = L.island_class0[c];
            A.n = L.island_class0[c + 1] - L.island_class0[c];
            HIP_TRY(mg_launch_sleep_pass(A, lanes[c], st));
        }
    }
    if (R.crep) {
        HIP_TRY(mg_launch_contact_compact(contact_args(s), st));
        s->crep_valid = true;
    }
    // the force sensors' readings, before the applied wrenches are cleared
    if (R.n_sens > 0) HIP_TRY(mg_launch_force_sensor(sensor_args(s, P), st));
    if (s->ext_pending) {
        HIP_TRY(hipMemsetAsync(s->d_ext, 0, (size_t)s->layout.nb * 6 * sizeof(float), st));
        s->ext_pending = false;
    }
    mg_timer = nullptr;
    if (!s->capturing) {
        if (timed) {
            HIP_TRY(hipEventRecord(s->ev_end, st));
            s->kern_n[slot] = timer.used;
            s->kern_miss[slot] = timer.missed;
            s->ring_n++;
        }
        s->timed_step = timed;
        s->last_stream = st;
        s->stepped = true;
    }
    return MG_OK;
}

int32_t mg_fetch_results(mg_sim* s, int32_t wait) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (wait && s->stepped && !s->capturing) {
        if (s->timed_step) HIP_TRY(hipEventSynchronize(s->ev_end));
        else HIP_TRY(hipStreamSynchronize(s->last_stream));
    }
    return MG_OK;
}

int32_t mg_fetch_host_state(mg_sim* s, float* dst, int32_t parts, void* stream) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!dst && parts) return fail(MG_ERR_ARG, "null destination");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(MG_ERR_STATE, "mg_fetch_host_state while capturing");
    if (int rc_ = flush_root(s, st)) return rc_;
    // [na][13] roots, [nb][13] bodies, [nd][2] DOFs, [nb][3] contact forces; the
    // parts asked for are gathered and the span covering them copied at once
    const size_t off[5] = {0, (size_t)s->layout.na * MG_STATE_N, (size_t)(s->layout.na + s->layout.nb) * MG_STATE_N,
                           (size_t)(s->layout.na + s->layout.nb) * MG_STATE_N + (size_t)s->layout.nd * 2,
                           (size_t)(s->layout.na + s->layout.nb) * MG_STATE_N + (size_t)s->layout.nd * 2 + (size_t)s->layout.nb * 3};
    // zero-copy when dst is the sim's own mapped stage (mg_host_stage): the parts
    // the last simulate wrote are already there, the others are gathered into it
    const bool alias = s->h_stage && dst == s->h_stage && s->h_stage_n >= off[4];
    if (!alias && s->host_out_n < off[4]) {   // the output stage (simulate writes into it from now on)
        s->host_out_n = 0;
        s->fuse.stage_freed(s->d_host_out);
        HIP_TRY(s->d_host_out.alloc(off[4]));
        s->host_out_n = off[4];
    }
    float* base = alias ? s->d_stage_alias : s->d_host_out;
    // parts the last simulate wrote there, with no state change since: no gather
    const int need = s->fuse.fetch(base) | 8;
    int lo = -1, hi = -1;
    for (int k = 0; k < 4; ++k) {
        if (!((parts >> k) & 1) || off[k + 1] == off[k]) continue;
        if (lo < 0) lo = k;
        hi = k;
        float* d = base + off[k];
        if (!((need >> k) & 1)) continue;
        if (k == 0) HIP_TRY(mg_launch_gather_rows(s->d_state, s->layout.nb, MG_STATE_N, s->d_actor_root, s->layout.na, d, st));
        if (k == 1) HIP_TRY(mg_launch_gather_rows(s->d_state, s->layout.nb, MG_STATE_N, s->d_perm, s->layout.nb, d, st));
        if (k == 2) HIP_TRY(mg_launch_gather_rows(s->d_dof, s->layout.nd, 2, nullptr, s->layout.nd, d, st));
        if (k == 3) HIP_TRY(mg_launch_gather_rows(s->d_cforce, s->layout.nb, 3, s->d_perm, s->layout.nb, d, st));
    }
    if (lo >= 0 && !alias)
        HIP_TRY(hipMemcpyAsync(dst + off[lo], s->d_host_out + off[lo], (off[hi + 1] - off[lo]) * sizeof(float),
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MG_OK;
}

int32_t mg_set_light(mg_sim* s, const mg_light* light) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!light) {
        s->has_light = false;
        return MG_OK;
    }
    const float* d = light->dir;
    if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > 0.0f)) return fail(MG_ERR_ARG, "zero light direction");
    s->light = *light;
    s->has_light = true;
    return MG_OK;
}

// ---- rigid-body attractors (mg_attractor.h) ----------------------------------
// attractor a's device record
static void attr_record(const mg_attractor& a, float* r) {
    for (int k = 0; k < MG_ATTR_N; ++k) r[k] = 0.0f;
    r[0] = (float)(a.axes & 63);
    r[1] = a.stiffness;
    r[2] = a.damping;
    for (int k = 0; k < 3; ++k) { r[3 + k] = a.offset_p[k]; r[10 + k] = a.target_p[k]; }
    for (int k = 0; k < 4; ++k) { r[6 + k] = a.offset_q[k]; r[13 + k] = a.target_q[k]; }
}

int32_t mg_set_attractors(mg_sim* s, const mg_attractor* host, int32_t n) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (n < 0 || (n > 0 && !host)) return fail(MG_ERR_ARG, "bad attractor table");
    if (int rc_ = refuse_captured(s, "attractor table changed")) return rc_;
    HIP_TRY(hipSetDevice(s->device));
    // the table is checked and routed (or its refusal kept for mg_simulate) by the plan
    MgRouteIn in = route_in(s);
    in.attrs = host; in.n_attr = n;
    MgRoute R;
    if (int rc_ = plan_route(s->layout, in, R)) return rc_;
    std::vector<int> wake;   // sleeping: the islands of the table's bodies
    for (int i = 0; i < n; ++i)
        if (s->layout.body_island[s->layout.perm[host[i].body]] >= 0) wake.push_back(s->layout.body_island[s->layout.perm[host[i].body]]);
    // the new state is built apart — fresh device buffers — and committed at the
    // end, so an error leaves the sim's table as it was
    DevBuf<int> d_idx, d_split;   // freed unless committed
    DevBuf<float> d_attr;
    HostBuf<float> h_attr;
    HIP_TRY(d_idx.upload(R.attr_idx));
    if (!R.split.empty()) HIP_TRY(d_split.upload(R.split));
    if (n > 0) {
        HIP_TRY(d_attr.alloc((size_t)n * MG_ATTR_N));
        HIP_TRY(h_attr.alloc((size_t)n * MG_ATTR_N, false));
        for (int i = 0; i < n; ++i) attr_record(host[i], h_attr + (size_t)i * MG_ATTR_N);
    }
    if (!s->attr_ev) HIP_TRY(hipEventCreateWithFlags(&s->attr_ev, hipEventDisableTiming));
    // no step may still read the buffers this replaces
    HIP_TRY(hipDeviceSynchronize());
    // ---- commit (nothing below fails)
    s->attr_ev_pending = false;
    s->d_attr_idx = std::move(d_idx);
    s->d_artic_split = std::move(d_split);
    s->d_attr = std::move(d_attr);
    s->h_attr = std::move(h_attr);
    s->attrs.assign(host, host + n);
    s->route = std::move(R);
    s->attr_dirty = n > 0;
    return sleep_wake_sync(s, &wake);
}

int32_t mg_set_attractor_targets(mg_sim* s, const float* pose7, int32_t first, int32_t n) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (n < 0 || first < 0 || (long long)first + n > (long long)s->attrs.size() || (n > 0 && !pose7))
        return fail(MG_ERR_ARG, "attractor targets %d .. %d out of range (%zu attractors)", first, first + n - 1,
                    s->attrs.size());
    for (int i = 0; i < 7 * n; ++i)
        if (!std::isfinite(pose7[i])) return fail(MG_ERR_ARG, "attractor target %d is not finite", first + i / 7);
    if (n == 0) return MG_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (s->attr_ev_pending) {   // the last copy out of h_attr
        HIP_TRY(hipEventSynchronize(s->attr_ev));
        s->attr_ev_pending = false;
    }
    std::vector<int> wake;   // sleeping: the islands of the moved attractors' bodies
    for (int i = 0; i < n; ++i) {
        mg_attractor& a = s->attrs[first + i];
        for (int k = 0; k < 3; ++k) a.target_p[k] = pose7[7 * i + k];
        for (int k = 0; k < 4; ++k) a.target_q[k] = pose7[7 * i + 3 + k];
        attr_record(a, s->h_attr + (size_t)(first + i) * MG_ATTR_N);
        const int isl = s->layout.body_island[s->layout.perm[a.body]];
        if (isl >= 0) wake.push_back(isl);
    }
    s->attr_dirty = true;
    return sleep_wake_sync(s, &wake);
}

int32_t mg_num_attractors(mg_sim* s) { return s ? (int32_t)s->attrs.size() : 0; }

float* mg_host_stage(mg_sim* s, int64_t nfloat) {
    if (!s || nfloat <= 0) { fail(MG_ERR_ARG, "null sim or empty stage"); return nullptr; }
    if (s->h_stage && s->h_stage_n >= (size_t)nfloat) return s->h_stage;
    if (hipSetDevice(s->device) != hipSuccess) { fail(MG_ERR_DEVICE, "hipSetDevice failed"); return nullptr; }
    if (s->h_stage) {
        (void)hipDeviceSynchronize();
        s->h_stage.reset();
        s->d_stage_alias = nullptr;
        s->h_stage_n = 0;
        s->fuse.stage_replaced(s->d_host_out);
    }
    HostBuf<float> h;
    if (h.alloc((size_t)nfloat, true) != hipSuccess) {
        fail(MG_ERR_DEVICE, "hipHostMalloc of the host stage failed");
        return nullptr;
    }
    float* d = nullptr;
    if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess || !d) {
        fail(MG_ERR_DEVICE, "hipHostGetDevicePointer of the host stage failed");
        return nullptr;
    }
    std::memset(h, 0, (size_t)nfloat * sizeof(float));
    s->h_stage = std::move(h);
    s->d_stage_alias = d;
    s->h_stage_n = (size_t)nfloat;
    return s->h_stage;
}

int32_t mg_set_fusion(mg_sim* s, int32_t flags) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    return s->fuse.set_flags(flags);
}

int32_t mg_bind_refresh_targets(mg_sim* s, float* root_dst, float* rigid_body_dst) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    s->fuse.bind(root_dst, rigid_body_dst);
    return MG_OK;
}

int32_t mg_bind_dof_refresh_target(mg_sim* s, float* dof_dst) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    s->fuse.bind_dof(dof_dst);
    return MG_OK;
}

int32_t mg_discard_pending_sets(mg_sim* s) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    s->fuse.discard();
    return MG_OK;
}

int32_t mg_step_out_supported(mg_sim* s) { return s && s->uploaded && s->route.step_writes_rows ? 1 : 0; }

int32_t mg_joint_friction_stats(mg_sim* s, int32_t out[3]) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!out) return fail(MG_ERR_ARG, "null output");
    out[0] = s->route.jfr_ndof;
    out[1] = s->route.jfr_lanes;
    out[2] = s->route.jfr_envs;
    return MG_OK;
}

// ---- sleeping ------------------------------------------------
int32_t mg_set_sleeping(mg_sim* s, float threshold, float window) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    const bool on = std::isfinite(threshold) && std::isfinite(window) && threshold > 0.0f && window > 0.0f;
    if (int rc_ = refuse_captured(s, "sleeping changed")) return rc_;
    if (s->uploaded) {
        HIP_TRY(hipSetDevice(s->device));
        MgRouteIn in = route_in(s);
        in.sleep = on;
        MgRoute R;
        if (int rc_ = plan_route(s->layout, in, R)) return rc_;
        // fresh buffers, committed at the end: timers at 0, anchors taken at the next pass
        SleepBufs B;
        if (on)
            if (int rc_ = sleep_alloc(s->layout, B)) return rc_;
        HIP_TRY(hipDeviceSynchronize());   // no pass may still read the buffers this replaces
        s->sleep = std::move(B);
        s->route = std::move(R);
    }
    s->sleep_on = on;
    s->sleep_threshold = on ? threshold : 0.0f;
    s->sleep_window = on ? window : 0.0f;
    return MG_OK;
}

int32_t mg_wake(mg_sim* s, const int32_t* actor_idx, int32_t n, int32_t idx_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (actor_idx && n < 0) return fail(MG_ERR_ARG, "negative index count");
    if (!sleeping(s) || (actor_idx && n == 0)) return MG_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const int* didx = actor_idx;
    if (actor_idx && idx_host) {
        if (int rc_ = ensure_stage(s, 0, (size_t)n)) return rc_;
        const void* src[1] = {actor_idx};
        const size_t bytes[1] = {(size_t)n * sizeof(int)};
        void* dst[1] = {s->d_stage_idx};
        if (int rc_ = pin_h2d(s, 1, src, bytes, dst, st)) return rc_;
        didx = s->d_stage_idx;
    }
    return sleep_wake(s, didx, n, st);
}

int32_t mg_sleep_state(mg_sim* s, int32_t* dst, int32_t dst_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    const int na = s->layout.na;
    if (na == 0) return MG_OK;
    if (!dst) return fail(MG_ERR_ARG, "null destination");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (!sleeping(s)) {   // nobody sleeps
        if (dst_host) std::memset(dst, 0, (size_t)na * sizeof(int32_t));
        else HIP_TRY(hipMemsetAsync(dst, 0, (size_t)na * sizeof(int32_t), st));
        return MG_OK;
    }
    int* d = dst_host ? (int*)s->sleep.d_idx : dst;
    HIP_TRY(mg_launch_sleep_actors(s->sleep.d_actor_island, na, s->sleep.d_asleep, d, st));
    if (dst_host) {
        HIP_TRY(hipMemcpyAsync(dst, d, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MG_OK;
}

int32_t mg_sleep_stats(mg_sim* s, int32_t out[3]) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!out) return fail(MG_ERR_ARG, "null output");
    out[0] = out[1] = out[2] = 0;
    if (!sleeping(s)) return MG_OK;
    const MgLayout& L = s->layout;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<int> asleep((size_t)L.n_island, 0);
    HIP_TRY(hipDeviceSynchronize());
    if (L.n_island > 0)
        HIP_TRY(hipMemcpy(asleep.data(), s->sleep.d_asleep, asleep.size() * sizeof(int), hipMemcpyDeviceToHost));
    out[0] = L.n_island;
    for (int a : asleep) out[1] += a != 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c) out[2] += L.island_class0[c + 1] > L.island_class0[c] ? 1 : 0;
    return MG_OK;
}

// ---- contact capacity report
int32_t mg_capacity_tracked(mg_sim* s) { return s && s->uploaded && cap_units(s->layout) > 0 ? 1 : 0; }

// the two reads' common opening: the sim's device, nothing while `st` is captured, then the wait
static int capacity_read_begin(mg_sim* s, hipStream_t st) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    HIP_TRY(hipSetDevice(s->device));
    if (capture_id(st)) return fail(MG_ERR_STATE, "the capacity report cannot be read while the stream is being captured");
    HIP_TRY(hipStreamSynchronize(st));
    return MG_OK;
}

int32_t mg_capacity_stats(mg_sim* s, int64_t out[MG_CAP_N], int32_t reset, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc_ = capacity_read_begin(s, st)) return rc_;
    if (!out) return fail(MG_ERR_ARG, "null output");
    unsigned long long h[MG_CAP_N];
    HIP_TRY(hipMemcpy(h, s->d_cap, sizeof h, hipMemcpyDeviceToHost));
    for (int k = 0; k < MG_CAP_N; ++k) out[k] = (int64_t)h[k];
    if (reset) {
        HIP_TRY(hipMemsetAsync(s->d_cap, 0, sizeof h, st));
        const int nu = cap_units(s->layout);
        if (nu > 0) HIP_TRY(hipMemsetAsync(s->d_cap_flags, 0, (size_t)nu * sizeof(int), st));
    }
    return MG_OK;
}

int32_t mg_capacity_env_flags(mg_sim* s, int32_t* dst_host, int32_t n_envs, void* stream) {
    if (int rc_ = capacity_read_begin(s, (hipStream_t)stream)) return rc_;
    const MgLayout& L = s->layout;
    if (!dst_host) return fail(MG_ERR_ARG, "null destination");
    if (n_envs != L.nenv) return fail(MG_ERR_ARG, "n_envs is %d, the model has %d envs", n_envs, L.nenv);
    std::fill(dst_host, dst_host + n_envs, 0);
    const int nu = cap_units(L);
    if (nu == 0) return MG_OK;
    std::vector<int> f((size_t)nu);
    HIP_TRY(hipMemcpy(f.data(), s->d_cap_flags, (size_t)nu * sizeof(int), hipMemcpyDeviceToHost));
    // unit -> env from the plan's mirrors
    auto put = [&](int env, int v) {
        if (v && env >= 0 && env < n_envs) dst_host[env] |= v;
    };
    for (int k = 0; k < L.n_pile; ++k) put(L.pile_env[k], f[k]);
    for (size_t k = 0; k < L.cenv_row.size(); ++k) put(L.cenv_env[k], f[cap_env0(L) + L.cenv_row[k]]);
    for (int i = 0; i < L.nf_rigid - L.nf1; ++i) put(L.slot_env[L.nf1 + i], f[cap_rigid0(L) + i]);
    return MG_OK;
}

int32_t mg_last_set_deferred(mg_sim* s) { return s ? s->fuse.last_set_deferred : 0; }

int32_t mg_set_kernel_timing(mg_sim* s, int32_t on) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    const int32_t prev = s->timing ? 1 : 0;
    s->timing = on != 0;
    return prev;
}

float mg_last_step_ms(mg_sim* s) {
    if (!s || !s->stepped || !s->timed_step) return -1.0f;
    if (hipEventSynchronize(s->ev_end) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, s->ev_begin, s->ev_end) != hipSuccess) return -1.0f;
    return ms;
}

int32_t mg_step_time_stats(mg_sim* s, int32_t n, float* avg_ms, float* min_ms, float* max_ms) {
    if (!s || n <= 0) return fail(MG_ERR_ARG, "bad arguments");
    if (s->ring_n == 0) return fail(MG_ERR_STATE, "no simulate() recorded");
    long long avail = s->ring_n < mg_sim::kRing ? s->ring_n : mg_sim::kRing;
    if (n > avail) n = (int32_t)avail;
    double sum = 0.0;
    float lo = 1e30f, hi = 0.0f;
    for (int32_t k = 0; k < n; ++k) {
        const int slot = (int)((s->ring_n - 1 - k) % mg_sim::kRing);
        HIP_TRY(hipEventSynchronize(s->ring_e[slot]));
        // sum of the step kernels' own durations (dispatch timestamps)
        float ms = 0.0f;
        for (int j = 0; j < s->kern_n[slot]; ++j) {
            float kms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&kms, s->kern_b[slot][j], s->kern_e[slot][j]));
            ms += kms;
        }
        sum += ms;
        lo = ms < lo ? ms : lo;
        hi = ms > hi ? ms : hi;
    }
    if (avg_ms) *avg_ms = (float)(sum / n);
    if (min_ms) *min_ms = lo;
    if (max_ms) *max_ms = hi;
    return n;
}

int32_t mg_step_untimed_launches(mg_sim* s, int32_t n) {
    if (!s || n <= 0) return fail(MG_ERR_ARG, "bad arguments");
    if (s->ring_n == 0) return fail(MG_ERR_STATE, "no simulate() recorded");
    const long long avail = s->ring_n < mg_sim::kRing ? s->ring_n : mg_sim::kRing;
    if (n > avail) n = (int32_t)avail;
    int32_t most = 0;
    for (int32_t k = 0; k < n; ++k) {
        const int slot = (int)((s->ring_n - 1 - k) % mg_sim::kRing);
        most = std::max(most, s->kern_miss[slot]);
    }
    return most;
}

// diagnostics (tests/test_franka_gpu.py, tools/diag_franka_env.py): coupled
// env k's contact table (k_env_np's output of the last substep run): the
// group's base and record size are the library's, so callers hard-code neither
int32_t mg_debug_copy_env_ctab(mg_sim* s, int32_t k, float* dst, int32_t cap) {
    if (!s || !s->uploaded || !s->d_env_ctab || !dst) return fail(MG_ERR_ARG, "bad arguments");
    if (k < 0 || k >= (int32_t)s->layout.cenv_ctab_off.size()) return fail(MG_ERR_ARG, "no such coupled env");
    const int32_t n = s->layout.cenv_ctab_n[k];
    if (cap < n) return fail(MG_ERR_ARG, "dst holds fewer floats than the env's contact table");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst, s->d_env_ctab + s->layout.cenv_ctab_off[k], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

// diagnostics (tests/test_step_out_chain_gpu.py): per articulation group the
// facts that choose its chain-kernel form (mg_chain.hip mg_launch_artic_chain)
int32_t mg_debug_artic_groups(mg_sim* s, int32_t* out, int32_t cap) {
    if (!s || !s->uploaded || (!out && cap > 0)) return fail(MG_ERR_ARG, "bad arguments");
    const int32_t n = (int32_t)s->layout.groups.size();
    for (int32_t i = 0; i < n && (i + 1) * MG_DEBUG_GROUP_N <= cap; ++i) {
        const MgArticGroup& g = s->layout.groups[i];
        int32_t* r = out + (size_t)i * MG_DEBUG_GROUP_N;
        r[0] = g.nl; r[1] = g.step_count; r[2] = g.chain; r[3] = g.uni_mass ? 1 : 0;
        r[4] = s->groups[i].uni_dof ? 1 : 0; r[5] = g.aff; r[6] = g.out_aff; r[7] = s->layout.step_out_ok ? 1 : 0;
    }
    return n;
}

// diagnostics (tests/test_layout.py): the layout plan of a model, with no sim
// and no device — a window onto MgLayout (mg_layout.h)
struct mg_layout {
    MgLayout L;
    std::vector<int32_t> scalars, island_class;
};
mg_layout* mg_debug_plan_layout(const mg_sim_params* p, const mg_model* m) {
    if (!p || !m) { fail(MG_ERR_ARG, "null argument"); return nullptr; }
    mg_layout* h = new mg_layout();
    std::string err;
    if (int rc_ = mg_plan_layout(*p, *m, layout_sizes(), h->L, err)) {
        fail(rc_, "%s", err.c_str());
        delete h;
        return nullptr;
    }
    const MgLayout& L = h->L;
    h->scalars = {L.nb, L.na, L.nd, L.nf, L.nf1, L.nf_rigid, L.n_coupled, L.n_pile, L.max_actor_dofs,
                  L.roots_free ? 1 : 0, L.step_out_ok ? 1 : 0, (int32_t)L.groups.size(), (int32_t)L.env_groups.size()};
    for (const MgArticGroup& g : L.groups)
        h->scalars.insert(h->scalars.end(), {g.chain, g.aff, g.aff_b0, g.aff_d0, g.aff_ds, g.out_aff, g.out_g0, g.out_r0,
                                             g.offset, g.count, g.step_offset, g.step_count, g.uni_mass ? 1 : 0, g.nl});
    for (const MgEnvGroup& g : L.env_groups)
        h->scalars.insert(h->scalars.end(), {g.tmpl, g.wide, g.max_free, g.offset, g.count});
    h->island_class = {L.n_island, L.island_class0[1], L.island_class0[2]};
    return h;
}
int32_t mg_debug_layout_table(const mg_layout* h, int32_t which, const void** data, int64_t* count) {
    if (!h || !data || !count) return fail(MG_ERR_ARG, "bad arguments");
    const MgLayout& L = h->L;
    auto give = [&](const auto& v) { *data = v.data(); *count = (int64_t)v.size(); return MG_OK; };
    switch (which) {
        case MG_LAYOUT_SCALARS: return give(h->scalars);
        case MG_LAYOUT_PERM: return give(L.perm);
        case MG_LAYOUT_ARTIC_SORTED: return give(L.artic_sorted);
        case MG_LAYOUT_ARTIC_STEP: return give(L.artic_step);
        case MG_LAYOUT_ENV_FLAT: return give(L.env_flat);
        case MG_LAYOUT_PAIRS: return give(L.pairs);
        case MG_LAYOUT_PILE_ROWS: return give(L.pile_rows);
        case MG_LAYOUT_PILE_BODY: return give(L.pile_body);
        case MG_LAYOUT_PILE_SLOTS: return give(L.pile_slots);
        case MG_LAYOUT_PILE_PAIRS: return give(L.pile_pairs);
        case MG_LAYOUT_CENV_ROW: return give(L.cenv_row);
        case MG_LAYOUT_CENV_CTAB_OFF: return give(L.cenv_ctab_off);
        case MG_LAYOUT_FREE_FLAGS: return give(L.free_flags);
        case MG_LAYOUT_BODY_ISLAND: return give(L.body_island);
        case MG_LAYOUT_ACTOR_ISLAND: return give(L.actor_island);
        case MG_LAYOUT_ISLAND_BODY0: return give(L.island_body0);
        case MG_LAYOUT_ISLAND_BODY: return give(L.island_body);
        case MG_LAYOUT_ISLAND_DOF0: return give(L.island_dof0);
        case MG_LAYOUT_ISLAND_DOF: return give(L.island_dof);
        case MG_LAYOUT_ISLAND_CLASS: return give(h->island_class);
        case MG_LAYOUT_BODY_K: return give(L.body_k);
        default: return fail(MG_ERR_ARG, "no layout table %d", which);
    }
}
void mg_debug_free_layout(mg_layout* h) { delete h; }

// the S3 cube-pick controller (csrc/mg_ctrl.hip): independent of any sim, on
// the caller's stream (torch's current stream: ordered with the refreshes that
// filled its inputs and the sets that read its outputs)
int32_t mg_cube_pick_step(const mg_cube_pick_args* a, void* stream) {
    if (!a || a->n < 0) return fail(MG_ERR_ARG, "bad arguments");
    if (a->n == 0) return MG_OK;
    if (!a->rb || !a->box_row || !a->hand_row || !a->dof || !a->dof_row0 || !a->jac || (a->osc && !a->mm) ||
        !a->init_pos || !a->init_rot || !a->default_dof_pos || !a->hand_restart || !a->pos_action ||
        !a->effort_action)
        return fail(MG_ERR_ARG, "null tensor");
    HIP_TRY(mg_launch_cube_pick(*a, (hipStream_t)stream));
    return MG_OK;
}

// diagnostics (tests/test_rcp_pairs_gpu.py): the paired reciprocal of the
// free-body step's row constants over a device array, on the current device
int32_t mg_debug_rcp_pairs(const float* d, float* out, int32_t n) {
    if (n < 0 || (n > 0 && (!d || !out))) return fail(MG_ERR_ARG, "bad arguments");
    HIP_TRY(mg_launch_rcp_pairs(d, out, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return MG_OK;
}

int32_t mg_last_rigid_form(mg_sim* s) {
    if (s)
        for (const MgBuild& b : s->builds)
            if (b.kernel == MG_K_RIGID_STEP1) return mg_rigid_form_public(b.form);
    return -1;
}

int32_t mg_debug_step_builds(mg_sim* s, int32_t* out, int32_t cap) {
    if (!s || cap < 0 || (cap > 0 && !out)) return fail(MG_ERR_ARG, "mg_debug_step_builds: null sim or buffer");
    for (size_t i = 0; i < s->builds.size() && (int32_t)i < cap; ++i) {
        const MgBuild& b = s->builds[i];
        const int32_t row[MG_STEP_BUILD_N] = {b.kernel, b.size, (int32_t)b.form};
        std::memcpy(out + i * MG_STEP_BUILD_N, row, sizeof row);
    }
    return (int32_t)s->builds.size();
}
int32_t mg_num_free_bodies(mg_sim* s) { return s ? s->layout.nf : 0; }
int32_t mg_num_articulations(mg_sim* s) { return s ? s->layout.nartic : 0; }
int32_t mg_num_coupled_envs(mg_sim* s) { return s ? s->layout.n_coupled : 0; }
int32_t mg_num_pile_envs(mg_sim* s) { return s ? s->layout.n_pile : 0; }

int32_t mg_refresh_actor_root_state(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc_ = flush_root(s, st)) return rc_;
    const unsigned long long cid = capture_id(st);
    const MgFusion::Refresh r = s->fuse.refresh(MG_PART_ROOT, dst, dst_host, cid, s->layout.na > 0);
    if (r.how == MG_REFRESH_SKIP) return MG_OK;   // written by the step kernel
    if (r.how == MG_REFRESH_PAIRED) {   // the bound root and rigid-body tensors in one launch
        HIP_TRY(mg_launch_gather_rb_root(s->d_state, s->layout.nb, MG_STATE_N, s->d_perm, s->layout.nb, r.rb, s->d_body_actor,
                                         dst, st));
        s->fuse.refreshed(r, cid);
        return MG_OK;
    }
    return refresh_rows(s, s->d_state, s->layout.nb, MG_STATE_N, s->d_actor_root, s->layout.na, dst, dst_host, st);
}
int32_t mg_refresh_rigid_body_state(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    if (!s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc_ = flush_root(s, st)) return rc_;
    const unsigned long long cid = capture_id(st);
    const MgFusion::Refresh r = s->fuse.refresh(MG_PART_RB, dst, dst_host, cid, s->layout.na > 0);
    if (r.how == MG_REFRESH_SKIP) return MG_OK;   // served by the paired gather / the step kernel
    const int rc = refresh_rows(s, s->d_state, s->layout.nb, MG_STATE_N, s->d_perm, s->layout.nb, dst, dst_host, st);
    if (rc == MG_OK) s->fuse.refreshed(r, cid);
    return rc;
}
int32_t mg_refresh_dof_state(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    const MgFusion::Refresh r =
        s->fuse.refresh(MG_PART_DOF, dst, dst_host, capture_id((hipStream_t)stream), s->layout.na > 0);
    if (r.how == MG_REFRESH_SKIP) return MG_OK;   // written by the step kernel
    return refresh_rows(s, s->d_dof, s->layout.nd, 2, nullptr, s->layout.nd, dst, dst_host, (hipStream_t)stream);
}

// ---- DOF force tensor --------------------------------------
int32_t mg_enable_dof_forces(mg_sim* s, const int32_t* actor_on, int32_t n_actors) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (actor_on && n_actors != s->layout.na)
        return fail(MG_ERR_ARG, "DOF force flags for %d actors, the model has %d", n_actors, s->layout.na);
    if (int rc_ = refuse_captured(s, "DOF force reporting changed")) return rc_;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<float> on((size_t)std::max(s->layout.nd, 1), 0.0f);
    int n = 0;
    if (actor_on)
        for (int a = 0; a < s->layout.na; ++a)
            if (actor_on[a])
                for (int d = s->layout.actor_dof[a]; d < s->layout.actor_dof[a + 1]; ++d) { on[d] = 1.0f; ++n; }
    MgRouteIn in = route_in(s);
    in.dof_frc_n = n;
    MgRoute R;
    if (int rc_ = plan_route(s->layout, in, R)) return rc_;
    // rows of actors that stop reporting, or that no kernel steps, read 0
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(s->d_dof_frc, 0, (size_t)std::max(s->layout.nd, 1) * sizeof(float)));
    if (s->layout.nd > 0)
        HIP_TRY(hipMemcpy(s->d_dof_frc + s->layout.nd, on.data(), (size_t)s->layout.nd * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    s->route = std::move(R);
    return MG_OK;
}

int32_t mg_refresh_dof_force(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!dst && s->layout.nd > 0) return fail(MG_ERR_ARG, "null destination");
    HIP_TRY(hipSetDevice(s->device));
    if (s->layout.nd == 0) return MG_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!dst_host) {
        HIP_TRY(mg_launch_dof_force_rows(s->d_dof_frc, s->d_dof_frc + s->layout.nd, s->layout.nd, dst, st));
        return MG_OK;
    }
    if (int rc = ensure_stage(s, (size_t)s->layout.nd, 0)) return rc;
    HIP_TRY(mg_launch_dof_force_rows(s->d_dof_frc, s->d_dof_frc + s->layout.nd, s->layout.nd, s->d_stage, st));
    HIP_TRY(hipMemcpyAsync(dst, s->d_stage, (size_t)s->layout.nd * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MG_OK;
}

int32_t mg_num_dof_force_dofs(mg_sim* s) { return s ? s->route.dof_frc_n : 0; }

// ---- force sensors -------------------------------------------
int32_t mg_set_force_sensors(mg_sim* s, const mg_force_sensor* host, int32_t n) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (n < 0 || (n > 0 && !host)) return fail(MG_ERR_ARG, "bad force sensor table");
    if (int rc_ = refuse_captured(s, "force sensor table changed")) return rc_;
    HIP_TRY(hipSetDevice(s->device));
    // the table is checked, packed for the kernels and routed (or its refusal kept) by the plan
    MgRouteIn in = route_in(s);
    in.sensors = host; in.n_sens = n;
    MgRoute R;
    if (int rc_ = plan_route(s->layout, in, R)) return rc_;
    // fresh device buffers, committed at the end: an error leaves the table as it was
    HIP_TRY(hipDeviceSynchronize());
    SensBufs B;
    if (R.n_sens > 0) {
        hipError_t e = B.d_sens_i.upload(R.si);
        if (e == hipSuccess) e = B.d_sens_f.upload(R.sf);
        if (e == hipSuccess) e = B.d_sart_i.upload(R.sart);
        // no frame held yet: every articulation's first frame reads 0
        if (e == hipSuccess) e = B.d_sens_flag.zero((size_t)2 * R.n_sart + 1);
        if (e == hipSuccess) e = B.d_sens_hist.zero((size_t)12 * R.sens_nhb);
        if (e == hipSuccess) e = B.d_sens_save.zero((size_t)R.sens_nsave);
        if (e == hipSuccess) e = B.d_sens_out.zero((size_t)6 * R.n_sens);
        if (e == hipSuccess && !s->d_ctorque) e = s->d_ctorque.zero((size_t)3 * std::max(s->layout.nb, 1));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return fail(MG_ERR_DEVICE, "force sensor table: %s", hipGetErrorString(e));
    }
    static_cast<SensBufs&>(*s) = std::move(B);
    s->sensors.assign(host, host + n);
    s->route = std::move(R);
    return MG_OK;
}

int32_t mg_refresh_force_sensor(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!s->route.sens_refusal.empty()) return fail(MG_ERR_UNSUPPORTED, "%s", s->route.sens_refusal.c_str());
    if (s->route.n_sens == 0) return MG_OK;
    if (!dst) return fail(MG_ERR_ARG, "null destination");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)s->route.n_sens * 6 * sizeof(float);
    HIP_TRY(hipMemcpyAsync(dst, s->d_sens_out, bytes, dst_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (dst_host) HIP_TRY(hipStreamSynchronize(st));
    return MG_OK;
}

int32_t mg_num_force_sensors(mg_sim* s) { return s ? (int32_t)s->sensors.size() : 0; }

// ---- rigid contact list ----------------------------------------
int32_t mg_set_contact_reporting(mg_sim* s, int32_t on, int32_t capacity) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (capacity < 0) return fail(MG_ERR_ARG, "negative contact capacity %d", capacity);
    if (int rc_ = refuse_captured(s, "contact reporting changed")) return rc_;
    HIP_TRY(hipSetDevice(s->device));
    MgRouteIn in = route_in(s);
    MgRoute R_off, R_on;
    in.crep = false;
    if (int rc_ = plan_route(s->layout, in, R_off)) return rc_;
    in.crep = true;
    if (int rc_ = plan_route(s->layout, in, R_on)) return rc_;
    HIP_TRY(hipDeviceSynchronize());
    static_cast<CrepBufs&>(*s) = CrepBufs();
    s->route = std::move(R_off);
    s->crep_valid = false;
    s->crep_capacity = 0;
    if (!on) return MG_OK;
    const MgLayout& L = s->layout;
    const int nfree = L.nf_rigid, ncenv = L.n_coupled, npile = L.n_pile, nown = nfree + ncenv + npile;
    const int cenv_cap = 2 * MG_ENV_MAXCT_WIDE;
    const long long worst = (long long)nfree * MG_CREP_FREE_CAP + (long long)ncenv * cenv_cap +
                            (long long)npile * MG_PILE_MAXPT;
    if (worst > (1ll << 30)) return fail(MG_ERR_UNSUPPORTED, "contact reporting: %lld staged entries", worst);
    const int cap = capacity > 0 ? capacity : (int)std::max(worst, 1ll);
    // fresh buffers, committed at the end: a failure leaves reporting off and nothing half set
    CrepBufs B;
    HIP_TRY(B.d_crep_free.alloc((size_t)std::max(nfree, 1) * MG_CREP_FREE_CAP * MG_CREP_N));
    HIP_TRY(B.d_crep_free_n.zero((size_t)nfree));
    HIP_TRY(B.d_crep_cenv.alloc((size_t)std::max(ncenv, 1) * cenv_cap * MG_CREP_N));
    HIP_TRY(B.d_crep_cenv_n.zero((size_t)ncenv));
    HIP_TRY(B.d_crep_col.upload(L.cenv_row.data(), (size_t)ncenv));
    HIP_TRY(B.d_crep_pile.alloc((size_t)std::max(npile, 1) * MG_PILE_MAXPT * MG_CREP_N));
    HIP_TRY(B.d_crep_pile_n.zero((size_t)npile));
    // owner -> env: free bodies are their own actors' roots (owner = storage
    // slot), then the coupled envs and the pile envs, each by env index
    std::vector<int> env(L.slot_env.begin(), L.slot_env.begin() + nfree);
    env.insert(env.end(), L.cenv_env.begin(), L.cenv_env.end());
    env.insert(env.end(), L.pile_env.begin(), L.pile_env.end());
    HIP_TRY(B.d_crep_env.upload(env));
    HIP_TRY(B.d_crep_blk.alloc((size_t)(nown + MG_CREP_BLOCK - 1) / MG_CREP_BLOCK + 1));
    HIP_TRY(B.d_crep_out.alloc((size_t)cap));
    HIP_TRY(B.d_crep_hdr.zero(2));
    if (!s->h_crep_hdr) {
        HostBuf<int> h;
        int* d = nullptr;
        HIP_TRY(h.alloc(2, true));
        HIP_TRY(hipHostGetDevicePointer((void**)&d, h, 0));
        s->h_crep_hdr = std::move(h);
        s->d_crep_hdr_alias = d;
    }
    s->h_crep_hdr[0] = 0;
    s->h_crep_hdr[1] = 0;
    HIP_TRY(hipDeviceSynchronize());
    static_cast<CrepBufs&>(*s) = std::move(B);
    s->crep_capacity = cap;
    s->route = std::move(R_on);
    return MG_OK;
}

int32_t mg_contact_reporting(mg_sim* s) { return s && s->route.crep ? 1 : 0; }

int32_t mg_refresh_rigid_contacts(mg_sim* s, mg_rigid_contact* dst, int32_t cap, int32_t dst_host, int32_t* total,
                                  void* stream) {
    if (total) *total = 0;
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (cap < 0 || (!dst && cap > 0)) return fail(MG_ERR_ARG, "bad destination");
    if (!s->route.crep || !s->crep_valid) return 0;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) return fail(MG_ERR_STATE, "mg_refresh_rigid_contacts while capturing");
    // the record count is the compaction's: wait for it, then copy that many
    HIP_TRY(hipStreamSynchronize(st));
    const int all = s->h_crep_hdr[0], stored = std::min(s->h_crep_hdr[1], s->crep_capacity);
    if (total) *total = all;
    const int n = std::max(std::min(stored, cap), 0);
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(dst, s->d_crep_out, (size_t)n * sizeof(mg_rigid_contact),
                               dst_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        if (dst_host) HIP_TRY(hipStreamSynchronize(st));
    }
    return n;
}

int32_t mg_refresh_net_contact_force(mg_sim* s, float* dst, int32_t dst_host, void* stream) {
    if (!s) return fail(MG_ERR_ARG, "null sim");
    return refresh_rows(s, s->d_cforce, s->layout.nb, 3, s->d_perm, s->layout.nb, dst, dst_host, (hipStream_t)stream);
}

int32_t mg_set_actor_root_state(mg_sim* s, const float* src, int32_t src_host, const int32_t* idx,
                                int32_t n_idx, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!src) return fail(MG_ERR_ARG, "null source tensor");
    if (idx && n_idx < 0) return fail(MG_ERR_ARG, "negative index count");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const float* dsrc;
    const int* didx;
    if (!idx)   // autowake: a full set wakes every island (an indexed one: below, its actors')
        if (int rc_ = sleep_wake(s, nullptr, 0, st)) return rc_;
    const MgFusion::Set f = s->fuse.set_root(src, src_host, idx != nullptr, s->layout.roots_free, capture_id(st));
    if (int rc_ = apply_root(s, f.first, st)) return rc_;
    if (f.how != MG_SET_NOW) s->set_st[0] = st;
    if (f.how == MG_SET_DEFER) return MG_OK;   // read by the next simulate
    if (f.how == MG_SET_DEFER_MAPPED) {
        // CPU pipeline, full set: copied at the call into the library's own buffer
        // (Isaac Gym's copy-at-set), read by the next simulate's step kernel like
        // a fused device set — or by the scatter a reader of the state issues first
        const size_t bytes = (size_t)s->layout.na * MG_STATE_N * sizeof(float);
        if (!s->h_root_in) {        // page-locked and device-mapped: the step kernel reads it over PCIe
            HostBuf<float> h;
            HIP_TRY(h.alloc(bytes / sizeof(float), true));
            HIP_TRY(hipHostGetDevicePointer((void**)&s->d_root_in_alias, h, 0));
            s->h_root_in = std::move(h);
            HIP_TRY(hipEventCreateWithFlags(&s->root_ev, hipEventDisableTiming));
        }
        if (s->root_ev_pending) HIP_TRY(hipEventSynchronize(s->root_ev));   // its last reader is done
        s->root_ev_pending = false;
        std::memcpy(s->h_root_in, src, bytes);
        s->fuse.root_mapped(s->d_root_in_alias);
        return MG_OK;
    }
    int rc = stage_src(s, src, src_host, (size_t)s->layout.na * MG_STATE_N, idx, n_idx, st, &dsrc, &didx);
    if (rc) return rc;
    if (idx && (rc = sleep_wake(s, didx, n_idx, st))) return rc;
    HIP_TRY(mg_launch_scatter_rows(dsrc, MG_STATE_N, s->d_actor_root, didx, idx ? n_idx : s->layout.na, s->layout.na,
                                   s->d_state, s->layout.nb, st));
    return MG_OK;
}

int32_t mg_set_rigid_body_state(mg_sim* s, const float* src, int32_t src_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!src) return fail(MG_ERR_ARG, "null source tensor");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const float* dsrc;
    const int* didx;
    if (int rc_ = apply_root(s, s->fuse.set_rigid_body(capture_id(st)), st)) return rc_;
    if (int rc_ = sleep_wake(s, nullptr, 0, st)) return rc_;
    int rc = stage_src(s, src, src_host, (size_t)s->layout.nb * MG_STATE_N, nullptr, 0, st, &dsrc, &didx);
    if (rc) return rc;
    // free bodies only: rows are selected through the free-body list
    HIP_TRY(mg_launch_scatter_rows(dsrc, MG_STATE_N, s->d_perm, s->d_free_global, s->layout.nf, s->layout.nb, s->d_state,
                                   s->layout.nb, st));
    return MG_OK;
}

int32_t mg_set_dof_state(mg_sim* s, const float* src, int32_t src_host, const int32_t* idx, int32_t n_idx,
                         void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    s->fuse.set_dof_state();
    return set_dof_columns(s, src, src_host, 2, s->d_dof, s->d_dof + s->layout.nd, idx, n_idx, (hipStream_t)stream);
}
// column k of the DOF targets; a device-resident full set is read by the next
// simulate's articulation kernels (MG_FUSE_DOF_TARGETS), else a scatter / copy
static int32_t set_dof_target(mg_sim* s, int k, const float* src, int32_t src_host, const int32_t* idx,
                              int32_t n_idx, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (s->layout.nd == 0) return MG_OK;
    if (!src) return fail(MG_ERR_ARG, "null source tensor");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->device));
    const MgFusion::Set f = s->fuse.set_target(k, src, src_host, idx != nullptr, capture_id(st));
    if (int rc_ = apply_tgt(s, k, f.first, st)) return rc_;
    if (f.how == MG_SET_DEFER) {
        s->set_st[1 + k] = st;
        return sleep_wake(s, nullptr, 0, st);   // autowake: a full set wakes every island
    }
    return set_dof_columns(s, src, src_host, 1, s->d_dof_tgt + (size_t)k * s->layout.nd, nullptr, idx, n_idx, st);
}
int32_t mg_set_dof_position_target(mg_sim* s, const float* src, int32_t src_host, const int32_t* idx,
                                   int32_t n_idx, void* stream) {
    return set_dof_target(s, 0, src, src_host, idx, n_idx, stream);
}
int32_t mg_set_dof_velocity_target(mg_sim* s, const float* src, int32_t src_host, const int32_t* idx,
                                   int32_t n_idx, void* stream) {
    return set_dof_target(s, 1, src, src_host, idx, n_idx, stream);
}
int32_t mg_set_dof_actuation_force(mg_sim* s, const float* src, int32_t src_host, const int32_t* idx,
                                   int32_t n_idx, void* stream) {
    return set_dof_target(s, 2, src, src_host, idx, n_idx, stream);
}

int32_t mg_set_dof_props(mg_sim* s, const float* props_host) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (s->layout.nd == 0) return MG_OK;
    if (!props_host) return fail(MG_ERR_ARG, "null props");
    HIP_TRY(hipSetDevice(s->device));
    // joint friction: the new routing is built apart and committed after the
    // table itself is copied; only a table that changes it needs the device idle
    std::vector<float> props(props_host, props_host + (size_t)s->layout.nd * MG_DOFPROP_N);
    MgRouteIn in = route_in(s);
    in.dof_props = props.data();
    MgRoute R;
    if (int rc_ = plan_route(s->layout, in, R)) return rc_;
    const bool changed = !R.same_launches(s->route);
    if (changed)
        if (int rc_ = refuse_captured(s, "DOF friction changed which kernels step the DOFs", "set")) return rc_;
    std::vector<float> dp = to_soa(props_host, s->layout.nd, MG_DOFPROP_N);
    DevBuf<int> d_split;
    if (changed) {
        if (!R.split.empty() && d_split.upload(R.split) != hipSuccess)
            return fail(MG_ERR_DEVICE, "joint friction routing: copy failed");
        HIP_TRY(hipDeviceSynchronize());   // the old launches read the old table and rows to their end
    }
    HIP_TRY(hipMemcpy(s->d_dof_props, dp.data(), dp.size() * sizeof(float), hipMemcpyHostToDevice));
    s->dof_props.swap(props);
    if (changed) s->d_artic_split = std::move(d_split);
    s->route = std::move(R);
    for (size_t gi = 0; gi < s->groups.size(); ++gi)
        if (s->layout.groups[gi].uni_mass) chain_uni_dof(props_host, s->layout.groups[gi], s->groups[gi]);
    HIP_TRY(chain_uni_upload(s));
    return sleep_wake_sync(s, nullptr);
}

int32_t mg_apply_rigid_body_force(mg_sim* s, const float* force, const float* torque, int32_t space,
                                  int32_t src_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (space != 0) return fail(MG_ERR_UNSUPPORTED, "only global-space forces are supported");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const float* parts[2] = {force, torque};
    for (int k = 0; k < 2; ++k) {
        if (!parts[k]) continue;
        const float* dsrc;
        const int* didx;
        int rc = stage_src(s, parts[k], src_host, (size_t)s->layout.nb * 3, nullptr, 0, st, &dsrc, &didx);
        if (rc) return rc;
        HIP_TRY(mg_launch_scatter_rows(dsrc, 3, s->d_perm, nullptr, s->layout.nb, s->layout.nb, s->d_ext + (size_t)k * 3 * s->layout.nb,
                                       s->layout.nb, st));
        if (src_host) HIP_TRY(hipStreamSynchronize(st));  // staging buffer is reused by the next part
    }
    s->ext_pending = true;
    if (sleeping(s))   // the islands of the bodies that now hold a force or a torque
        HIP_TRY(mg_launch_wake_ext(s->d_ext, s->layout.nb, s->sleep.d_body_island, s->sleep.d_timer, s->sleep.d_asleep, st));
    return MG_OK;
}

static int refresh_jac_mm(mg_sim* s, int32_t tmpl, float* jdst, float* mdst, int32_t dst_host, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!jdst && !mdst) return fail(MG_ERR_ARG, "null destination");
    const MgArticGroup* g = nullptr;
    for (const MgArticGroup& x : s->layout.groups)
        if (x.tmpl == tmpl) g = &x;
    if (!g) return fail(MG_ERR_ARG, "no articulation template %d", tmpl);
    const int nc = g->ndof + (g->fixed_base ? 0 : 6);
    if (nc > 32) return fail(MG_ERR_UNSUPPORTED, "jacobian / mass matrix of more than 32 generalized velocities");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t jper = (size_t)(g->nbody - (g->fixed_base ? 1 : 0)) * 6 * nc, mper = (size_t)nc * nc;
    const size_t jtot = jdst ? jper * g->count : 0, mtot = mdst ? mper * g->count : 0;
    float* jout = jdst;
    float* mout = mdst;
    if (dst_host) {
        int rc = ensure_stage(s, jtot + mtot, 0);
        if (rc) return rc;
        jout = jdst ? s->d_stage : nullptr;
        mout = mdst ? s->d_stage + jtot : nullptr;
    }
    MgArticArgs A{};
    A.na = g->count; A.nb = s->layout.nb; A.nd = s->layout.nd;
    A.artic_i = s->d_artic + (size_t)g->offset * MG_ARTIC_I_N;
    A.tmpl = g->tmpl; A.nl = g->nl; A.ndof = g->ndof; A.fixed_base = g->fixed_base; A.nbl = g->nbody;
    A.link_f = s->d_link_f + (size_t)g->first_link * MG_LINK_F_N;
    A.link_i = s->d_link_i + (size_t)g->first_link * MG_LINK_I_N;
    A.state = s->d_state; A.mass = s->d_mass;
    A.dof_pos = s->d_dof; A.dof_vel = s->d_dof + s->layout.nd;
    if (mtot > 0) HIP_TRY(hipMemsetAsync(mout, 0, mtot * sizeof(float), st));
    HIP_TRY(mg_launch_jacobian(A, jout, mout, st));
    if (dst_host) {
        if (jtot) HIP_TRY(hipMemcpyAsync(jdst, jout, jtot * sizeof(float), hipMemcpyDeviceToHost, st));
        if (mtot) HIP_TRY(hipMemcpyAsync(mdst, mout, mtot * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MG_OK;
}

int32_t mg_refresh_jacobian(mg_sim* s, int32_t tmpl, float* dst, int32_t dst_host, void* stream) {
    if (!dst) return fail(MG_ERR_ARG, "null destination");
    return refresh_jac_mm(s, tmpl, dst, nullptr, dst_host, stream);
}
int32_t mg_refresh_mass_matrix(mg_sim* s, int32_t tmpl, float* dst, int32_t dst_host, void* stream) {
    if (!dst) return fail(MG_ERR_ARG, "null destination");
    return refresh_jac_mm(s, tmpl, nullptr, dst, dst_host, stream);
}
int32_t mg_refresh_jacobian_mass_matrix(mg_sim* s, int32_t tmpl, float* jac, float* mm, int32_t dst_host,
                                        void* stream) {
    return refresh_jac_mm(s, tmpl, jac, mm, dst_host, stream);
}


// ---- camera sensors ---------------------------------------------------------

int32_t mg_set_render_bodies(mg_sim* s, const int32_t* env_body_first, const float* color, const int32_t* seg) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!env_body_first || !color || !seg) return fail(MG_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    const int ne = s->layout.nenv;
    if (env_body_first[0] != 0 || env_body_first[ne] != s->layout.nb) return fail(MG_ERR_ARG, "env_body_first must span [0, num_bodies]");
    std::vector<MgRShape> rs;
    std::vector<int> first(ne + 1, 0);
    for (int e = 0; e < ne; ++e) {
        first[e] = (int)rs.size();
        if (env_body_first[e + 1] < env_body_first[e]) return fail(MG_ERR_ARG, "env_body_first not monotone");
        for (int b = env_body_first[e]; b < env_body_first[e + 1]; ++b) {
            const int t = s->layout.body_tmpl[b];
            const int sh0 = s->layout.tbi[(size_t)t * MG_TBODY_I_N + 0], nsh = s->layout.tbi[(size_t)t * MG_TBODY_I_N + 1];
            for (int k = 0; k < nsh; ++k) {
                MgRShape r{};
                r.slot = s->layout.perm[b];
                r.shape = sh0 + k;
                r.seg = seg[b];
                r.r = color[3 * (size_t)b + 0]; r.g = color[3 * (size_t)b + 1]; r.b = color[3 * (size_t)b + 2];
                rs.push_back(r);
            }
        }
        if ((int)rs.size() - first[e] > MG_RENDER_MAX_SHAPES)
            return fail(MG_ERR_UNSUPPORTED, "env %d has %d shapes; a camera's env may hold at most %d", e,
                        (int)rs.size() - first[e], MG_RENDER_MAX_SHAPES);
    }
    first[ne] = (int)rs.size();
    s->d_rshapes.reset();
    s->d_env_shape_first.reset();
    HIP_TRY(s->d_rshapes.upload(rs));
    HIP_TRY(s->d_env_shape_first.upload(first));
    s->n_rshapes = (int)rs.size();
    s->render_ready = true;
    return MG_OK;
}

int32_t mg_snapshot_render_state(mg_sim* s, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->d_rstate) HIP_TRY(s->d_rstate.alloc((size_t)s->layout.nb * MG_STATE_N));
    if (int rc_ = flush_root(s, (hipStream_t)stream)) return rc_;
    HIP_TRY(hipMemcpyAsync(s->d_rstate, s->d_state, (size_t)s->layout.nb * MG_STATE_N * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    s->rstate_valid = true;
    return MG_OK;
}

int32_t mg_render_cameras(mg_sim* s, const mg_camera* cams, int32_t n, void* stream) {
    if (!s || !s->uploaded) return fail(MG_ERR_STATE, "sim has no uploaded model");
    if (!s->render_ready) return fail(MG_ERR_STATE, "mg_set_render_bodies was not called");
    if (!s->rstate_valid) return fail(MG_ERR_STATE, "no render snapshot (mg_snapshot_render_state)");
    if (n < 0 || (n > 0 && !cams)) return fail(MG_ERR_ARG, "bad camera list");
    if (n == 0) return MG_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const bool same = (int)s->cam_host.size() == n &&
                      std::memcmp(s->cam_host.data(), cams, (size_t)n * sizeof(mg_camera)) == 0;
    if (!same) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(st, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(MG_ERR_STATE, "camera table changed while the stream is being captured");
        std::vector<MgRenderCam> dev((size_t)n);
        long long blocks = 0;
        for (int i = 0; i < n; ++i) {
            const mg_camera& c = cams[i];
            if (c.env < 0 || c.env >= s->layout.nenv) return fail(MG_ERR_ARG, "camera %d: env %d out of range", i, c.env);
            if (c.width <= 0 || c.height <= 0 || (long long)c.width * c.height > (1ll << 30))
                return fail(MG_ERR_ARG, "camera %d: bad size %dx%d", i, c.width, c.height);
            if (c.body >= s->layout.nb) return fail(MG_ERR_ARG, "camera %d: body %d out of range", i, c.body);
            if (!(c.fx > 0.0f) || !(c.fy > 0.0f)) return fail(MG_ERR_ARG, "camera %d: bad focal length", i);
            MgRenderCam& d = dev[i];
            d.env = c.env; d.w = c.width; d.h = c.height;
            d.slot = c.body >= 0 ? s->layout.perm[c.body] : -1;
            d.follow = c.follow;
            d.blk0 = (int)blocks;
            const long long npx = (long long)c.width * c.height;
            d.nblk = (int)((npx + MG_RENDER_RUN - 1) / MG_RENDER_RUN);
            blocks += d.nblk;
            const auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
            d.vec = (npx % MG_RENDER_LANE_PX == 0) && al16(c.color) && al16(c.depth) && al16(c.seg);
            d.fx = c.fx; d.fy = c.fy; d.cx = c.cx; d.cy = c.cy;
            d.ifx = 1.0f / c.fx; d.ify = 1.0f / c.fy;
            d.near_plane = c.near_plane; d.far_plane = c.far_plane;
            for (int k = 0; k < 3; ++k) d.p[k] = c.p[k];
            for (int k = 0; k < 4; ++k) d.q[k] = c.q[k];
            d.color = c.color; d.depth = c.depth; d.seg = c.seg;
        }
        if (blocks > (1ll << 31) - 1) return fail(MG_ERR_ARG, "too many pixels in one render call");
        if (n > s->cam_cap) {
            s->cam_cap = 0;
            HIP_TRY(s->d_cams.alloc((size_t)n));
            s->cam_cap = n;
        }
        HIP_TRY(hipMemcpy(s->d_cams, dev.data(), (size_t)n * sizeof(MgRenderCam), hipMemcpyHostToDevice));
        s->cam_host.assign(cams, cams + n);
        s->cam_dev = dev;
        s->cam_blocks = (int)blocks;
    }
    MgRenderArgs A{};
    A.ncam = n; A.nb = s->layout.nb; A.cams = s->d_cams; A.state = s->d_rstate; A.shapes = s->d_shapes;
    A.hulls = s->d_hulls;
    A.uniform_nblk = s->cam_dev[0].nblk;
    for (int i = 1; i < n; ++i)
        if (s->cam_dev[i].nblk != A.uniform_nblk) { A.uniform_nblk = 0; break; }
    A.rshapes = s->d_rshapes; A.env_shape_first = s->d_env_shape_first;
    const mg_sim_params& p = s->params;
    A.has_ground = p.has_ground;
    for (int k = 0; k < 3; ++k) A.gn[k] = p.ground_normal[k];
    A.gpd = p.ground_distance;
    // camera frame (local axes): z-up sims look along +x with +z up (test11's
    // UAV camera, the controller's rot_coord3); y-up sims look along -z with +y
    // up (pinned by examples/graphics_images cam1, attached to a ball);
    // left = up x forward; light from above, a little off the up axis
    A.up_axis = p.up_axis == 0 ? 0 : 1;
    float lx = 0.3f, ly = 0.2f, lz = 1.0f;
    if (A.up_axis == 1) {
        A.fwd[0] = 1.0f; A.fwd[1] = 0.0f; A.fwd[2] = 0.0f;
        A.up[0] = 0.0f; A.up[1] = 0.0f; A.up[2] = 1.0f;
        A.left[0] = 0.0f; A.left[1] = 1.0f; A.left[2] = 0.0f;
    } else {
        A.fwd[0] = 0.0f; A.fwd[1] = 0.0f; A.fwd[2] = -1.0f;
        A.up[0] = 0.0f; A.up[1] = 1.0f; A.up[2] = 0.0f;
        A.left[0] = -1.0f; A.left[1] = 0.0f; A.left[2] = 0.0f;
        ly = 1.0f; lz = 0.2f;
    }
    for (int k = 0; k < 3; ++k) { A.lcol[k] = 0.7f; A.lamb[k] = 0.3f; }
    if (s->has_light) {
        lx = s->light.dir[0]; ly = s->light.dir[1]; lz = s->light.dir[2];
        for (int k = 0; k < 3; ++k) { A.lcol[k] = s->light.color[k]; A.lamb[k] = s->light.ambient[k]; }
    }
    const float inv = 1.0f / sqrtf(lx * lx + ly * ly + lz * lz);
    A.light[0] = lx * inv; A.light[1] = ly * inv; A.light[2] = lz * inv;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cap));
    const bool timed = s->timing && cap == hipStreamCaptureStatusNone;
    MgKernelTimer timer{};
    if (timed) {
        if (!s->rev_b) HIP_TRY(hipEventCreate(&s->rev_b));
        if (!s->rev_e) HIP_TRY(hipEventCreate(&s->rev_e));
        timer.start = &s->rev_b;
        timer.stop = &s->rev_e;
        timer.cap = 1;
        mg_timer = &timer;      // the launch carries the kernel's dispatch timestamps
    }
    const hipError_t e = mg_launch_render(A, s->cam_blocks, st);
    mg_timer = nullptr;
    HIP_TRY(e);
    s->rendered = timed;
    return MG_OK;
}

float mg_last_render_ms(mg_sim* s) {
    if (!s || !s->rendered) return -1.0f;
    if (hipEventSynchronize(s->rev_e) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, s->rev_b, s->rev_e) != hipSuccess) return -1.0f;
    return ms;
}

}  // extern "C"

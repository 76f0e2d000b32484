// mg_layout.h — the host-only layout plan of a model: every
// table and count mg_upload_model derives from (mg_sim_params, mg_model), as
// host vectors and scalars. Plain C++: no HIP, no device header. The constants
// of the device headers the planner needs arrive in MgLayoutSizes.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "../../include/migym.h"

// constants of mg_internal.h / mg_env.hip (filled by migym_capi.cpp)
struct MgLayoutSizes {
    int max_links, max_dofs;
    int env_i_n, env_maxf, env_maxs, env_slots_wide, env_free0, env_static0;
    int pile_i_n, pile_maxb, pile_st0, pile_maxpairs, pile_maxsh, pile_ground;
    int trec_n, trec_mass, obb_n;
    int env_ctab_floats, env_ctab_record_floats[2];   // mg_env_ctab_floats(), mg_env_ctab_record_floats(wide)
};

// articulation instances of one template
struct MgArticGroup {
    int chain;                     // serial chain with one DOF per moving link (MgArticArgs.chain)
    // the stepped instances' global first body / first DOF, and whether their
    // link mass rows and gravity flags agree (k_artic_chain's shared constants)
    std::vector<int> step_body0, step_dof0;
    bool uni_mass = false;
    int tmpl, first_link, nl, ndof, fixed_base;
    int nbody;                     // bodies per instance (nl minus the virtual links of ball joints)
    int offset, count;             // into the template-sorted instance list (all instances)
    int step_offset, step_count;   // into the list stepped by k_artic_chain / k_artic_lanes (uncoupled envs)
    // the stepped instances' rows are affine in the instance (MgArticArgs::aff),
    // and so are their fused-refresh rows (out_aff: rigid-body row og0 + a nl +
    // l, actor row or0 + a)
    int aff = 0, aff_b0 = 0, aff_d0 = 0, aff_ds = 0;
    int out_aff = 0, out_g0 = 0, out_r0 = 0;
};

// coupled envs (mg_env.hip) of one articulation template (tmpl -1: none)
struct MgEnvGroup {
    int tmpl, first_link, nl, ndof, floating;
    int wide;            // 64 lanes per env (mg_env.hip k_env_step<32, 64>), else 16
    int max_free;        // most free bodies of one env of the group (velocity slots)
    int offset, count;   // rows of env_flat
};

// what steps a body, for an attractor on it (mg_set_attractors)
enum AttrClass : char { ATTR_NONE = 0, ATTR_FREE, ATTR_LINK, ATTR_ENV_LINK, ATTR_ENV_FREE, ATTR_PILE };

// an articulation's first global body, first DOF, template, whether it steps in a coupled env
struct MgArticInfo { int g0, d0, tmpl, coupled; };

struct MgLayout {
    int nenv = 0, na = 0, nb = 0, nd = 0, ntb = 0, ns = 0, nf = 0, nartic = 0, ntl = 0;
    int max_actor_dofs = 0;
    int nf1 = 0;        // single-shape free bodies (storage slots 0..nf1-1)
    int nf_rigid = 0;   // free bodies of uncoupled envs (slots 0..nf_rigid-1), free-body kernel
    int n_coupled = 0, n_pile = 0;
    int nhull_floats = 0;
    bool roots_free = false;    // every actor root is a single-shape free body of the free-body kernel
    bool step_out_ok = false;   // every body is stepped by a kernel that writes its own tensor rows

    // internal storage order: free bodies (by launch group and template), each
    // articulation's links, the rest. order: slot -> global body (its first nf
    // entries: the free bodies); perm: global body -> slot
    std::vector<int> order, perm;
    std::vector<int> root_int;     // [na] slot of each actor's root
    std::vector<int> tmpl_int;     // [nb] template body of each slot
    std::vector<int> slot_actor;   // [nb] slot -> actor it is the root of, or -1
    std::vector<int> root_row;     // [nb] the same while roots_free holds its way, else partly -1
    std::vector<int> body_actor;   // [nb] global body -> actor it is the root of, or -1
    std::vector<std::array<int, 4>> slot_rec;   // [max(nb, 1)] {root_row, tmpl_int, order, slot_actor} (MgSlotRec)
    // free_flags[0] (box_only): every single-shape free body (slots 0..nf1-1)
    // has a box at the body origin with the body's orientation as its shape, or
    // no shape. A shape's type and pose are fixed at upload: no call rewrites
    // the shape or template records afterwards.
    std::vector<int> free_flags;
    std::vector<float> state0, mass0;           // SoA [13][nb], [12][nb] in storage order
    std::vector<float> trec;                    // [ntb][trec_n] compact template records (k_rigid_step1)
    std::vector<float> shape_obb;               // [max(ns, 1)][obb_n] shape-frame boxes
    std::vector<int> artic_sorted, artic_step;  // [..][MG_ARTIC_I_N] all instances by template / the stepped ones
    std::vector<MgArticGroup> groups;
    std::vector<MgEnvGroup> env_groups;
    std::vector<int> env_flat;                  // [n_coupled][env_i_n] coupled env rows, by group
    std::vector<int> pairs;                     // [..][4] candidate shape pairs of the coupled envs
    std::vector<int> pile_rows;                 // [n_pile][pile_i_n]
    std::vector<int> pile_body, pile_slots;     // the piles' free bodies (slots); [..][2] local shape slots
    std::vector<unsigned> pile_pairs;           // packed candidate pairs

    // mirrors later calls read (attractors, force sensors, contact list, joint friction)
    std::vector<char> body_class;               // global body -> AttrClass
    std::vector<int> body_grp, body_inst;       // a stepped articulation's link: group, stepped instance
    std::vector<int> body_artic;                // global body -> its articulation, -1: a single-body actor
    std::vector<MgArticInfo> artic_info;
    std::vector<int> slot_env;                  // [nb] slot of an actor root -> env
    std::vector<int> pile_env;                  // [n_pile] pile env -> env
    std::vector<int> cenv_env, cenv_row;        // coupled env k (env order) -> env, its row of env_flat
    std::vector<int> env_d0;                    // each row of env_flat's first DOF
    // coupled env k -> float offset / length of its contact-table record
    std::vector<long long> cenv_ctab_off;
    std::vector<int> cenv_ctab_n;
    // host copies of the model's tables
    std::vector<int> link_i, atmpl, body_tmpl, tbi, actor_dof;

    // Sleeping islands: the bodies that rest and wake as one. The moving actors
    // of a coupled or pile env form one island (every link of its articulation, every free body);
    // every other moving actor is an island of its own; static bodies have none (-1). Islands are
    // sorted by size class (1 body, 2..16, more: the lanes k_sleep_pass gives each) and within a
    // class by first storage slot, so the islands of the free-body kernel's bodies are 0..nf_rigid-1
    // in slot order and island i's body is slot i.
    int n_island = 0;
    int island_class0[4] = {0, 0, 0, 0};        // first island of each size class, and n_island
    std::vector<int> body_island;               // [nb] storage slot -> island, -1: static
    std::vector<int> actor_island;              // [na] actor -> island of its root, -1: static
    std::vector<int> island_body0, island_body; // CSR: island -> its storage slots (ascending)
    std::vector<int> island_dof0, island_dof;   // CSR: island -> its DOFs (ascending)
    // [nb] by storage slot: k_b = 4 r_b^2, r_b the body's bounding radius about its origin (the
    // largest |p_s| + extent_s over its shapes; a body without shapes takes its actor's largest)
    std::vector<float> body_k;
};

// Plans the layout of `m` under `p`. Returns MG_OK, or the error code with its
// message in `err` (then `out` is unspecified). Touches no device.
int mg_plan_layout(const mg_sim_params& p, const mg_model& m, const MgLayoutSizes& z, MgLayout& out, std::string& err);

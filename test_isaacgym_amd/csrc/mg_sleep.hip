// mg_sleep.hip — sleeping: resting islands freeze after the wake
// window and wake on a set.
//
//   k_sleep_pass     after a frame's last step launch: per island, restore (asleep),
//                    re-anchor (a body moved) or count towards the window (none did)
//   k_wake_actors    explicit wakes: by actor, by island, or all
//   k_wake_ext       the islands of bodies with an applied force or torque
//   k_sleep_actors   per actor: is its island asleep?
//
// An island is handled by 1, 16 or 64 lanes of one wavefront (its size class), so the
// island's OR is a ballot: no LDS, no atomics, nothing between blocks. A sleeping island
// is still stepped; the pass throws the step's result away. Numerics of §3.4:
// -ffp-contract=off, every operation rounded on its own, in the order written.
#include "mg_internal.h"

namespace {

// the OR of `v` over the G lanes that share an island (G consecutive lanes of the wavefront)
template <int G>
__device__ __forceinline__ bool group_or(bool v) {
    if constexpr (G == 1) {
        return v;
    } else {
        const unsigned long long m = __ballot(v);
        if constexpr (G == 64) return m != 0;
        return ((m >> (threadIdx.x & (64 - G))) & ((1ull << G) - 1)) != 0;
    }
}

// G lanes per island; lane l takes the island's bodies l, l + G, ... and its DOFs alike.
// With G = 1 consecutive lanes take consecutive islands, whose bodies are consecutive
// storage slots: every load and store of the SoA state is coalesced.
template <int G>
__global__ void __launch_bounds__(64) k_sleep_pass(MgSleepArgs A) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int k = t / G, lane = t % G;
    if (k >= A.n) return;   // whole lane groups leave together
    const int i = A.i0 + k;
    const size_t nb = (size_t)A.nb, nd = (size_t)A.nd;
    const int d0 = A.dof0[i], d1 = A.dof0[i + 1];
    const int timer = A.timer[i];
    if constexpr (G == 1) {
        // One body per island, and these islands come first: island i's CSR row is entry i. Both
        // poses are loaded before the island's state is looked at, so the pass is two dependent
        // memory trips (slot; poses) and its stores, whichever way the island goes.
        const int s = A.body[i];
        const bool asleep = A.asleep[i] != 0;
        float p[7], a[7];
        for (int f = 0; f < 7; ++f) { p[f] = A.state[f * nb + s]; a[f] = A.anchor[f * nb + s]; }
        const float kb = A.body_k[s];
        if (asleep) {
            for (int f = 0; f < 7; ++f) A.state[f * nb + s] = a[f];
        } else {
            const float dx = p[0] - a[0], dy = p[1] - a[1], dz = p[2] - a[2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const float c = ((p[3] * a[3] + p[4] * a[4]) + p[5] * a[5]) + p[6] * a[6];
            const float s2 = 1.0f - c * c;
            const bool moved = timer < 0 || d2 > A.tol2 || kb * s2 > A.tol2;
            const bool sleep = !moved && timer + 1 >= A.window;
            if (moved || sleep)
                for (int f = 0; f < 7; ++f) A.anchor[f * nb + s] = p[f];
            A.timer[i] = moved ? 0 : timer + 1;
            if (sleep) A.asleep[i] = 1;
            if (!sleep) return;
        }
        // asleep, or falling asleep: velocities 0; DOFs restored, or saved
        for (int f = 7; f < MG_STATE_N; ++f) A.state[f * nb + s] = 0.0f;
        for (int j = d0; j < d1; ++j) {
            const int d = A.dof[j];
            if (asleep) A.dofs[d] = A.dof_q[d];
            else A.dof_q[d] = A.dofs[d];
            A.dofs[nd + d] = 0.0f;
        }
        return;
    }
    const int b0 = A.body0[i], b1 = A.body0[i + 1];
    if (A.asleep[i]) {
        // asleep: the step's result is discarded
        for (int j = b0 + lane; j < b1; j += G) {
            const int s = A.body[j];
            for (int f = 0; f < 7; ++f) A.state[f * nb + s] = A.anchor[f * nb + s];
            for (int f = 7; f < MG_STATE_N; ++f) A.state[f * nb + s] = 0.0f;
        }
        for (int j = d0 + lane; j < d1; j += G) {
            const int d = A.dof[j];
            A.dofs[d] = A.dof_q[d];
            A.dofs[nd + d] = 0.0f;
        }
        return;
    }
    bool moved = timer < 0;   // no anchor yet: this pass takes it
    for (int j = b0 + lane; j < b1 && !moved; j += G) {
        const int s = A.body[j];
        const float dx = A.state[s] - A.anchor[s];
        const float dy = A.state[nb + s] - A.anchor[nb + s];
        const float dz = A.state[2 * nb + s] - A.anchor[2 * nb + s];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float c = ((A.state[3 * nb + s] * A.anchor[3 * nb + s] + A.state[4 * nb + s] * A.anchor[4 * nb + s]) +
                         A.state[5 * nb + s] * A.anchor[5 * nb + s]) +
                        A.state[6 * nb + s] * A.anchor[6 * nb + s];
        const float s2 = 1.0f - c * c;
        moved = d2 > A.tol2 || A.body_k[s] * s2 > A.tol2;
    }
    const bool any = group_or<G>(moved);
    const bool sleep = !any && timer + 1 >= A.window;
    if (any || sleep) {
        for (int j = b0 + lane; j < b1; j += G) {
            const int s = A.body[j];
            for (int f = 0; f < 7; ++f) A.anchor[f * nb + s] = A.state[f * nb + s];
            if (sleep)
                for (int f = 7; f < MG_STATE_N; ++f) A.state[f * nb + s] = 0.0f;
        }
    }
    if (sleep) {
        for (int j = d0 + lane; j < d1; j += G) {
            const int d = A.dof[j];
            A.dof_q[d] = A.dofs[d];
            A.dofs[nd + d] = 0.0f;
        }
    }
    if (lane == 0) {
        A.timer[i] = any ? 0 : timer + 1;
        if (sleep) A.asleep[i] = 1;
    }
}

__device__ __forceinline__ void wake(int i, int* timer, int* asleep) {
    asleep[i] = 0;
    if (timer[i] > 0) timer[i] = 0;   // < 0 stays: no anchor taken yet
}

__global__ void __launch_bounds__(64) k_wake_actors(const int* idx, int n, const int* table, int n_table, int n_island, int* timer,
                                              int* asleep) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    int v = idx ? idx[t] : t;
    if (table) {
        if (v < 0 || v >= n_table) return;
        v = table[v];
    }
    if (v < 0 || v >= n_island) return;
    wake(v, timer, asleep);
}

__global__ void __launch_bounds__(64) k_wake_ext(const float* ext, int nb, const int* body_island, int* timer, int* asleep) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nb) return;
    const int i = body_island[s];
    bool on = false;
    for (int f = 0; f < 6; ++f) on = on || ext[(size_t)f * nb + s] != 0.0f;
    if (i >= 0 && on) wake(i, timer, asleep);
}

__global__ void __launch_bounds__(64) k_sleep_actors(const int* actor_island, int na, const int* asleep, int* dst) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= na) return;
    const int i = actor_island[a];
    dst[a] = i >= 0 && asleep[i] != 0 ? 1 : 0;
}

}  // namespace

hipError_t mg_launch_sleep_pass(const MgSleepArgs& A, int lanes, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    if (lanes == 1 && A.i0 != 0) return hipErrorInvalidValue;   // single-body islands are islands 0 .. n - 1 (mg_layout.h)
    const dim3 grid((unsigned)(((long long)A.n * lanes + 63) / 64));
    if (lanes == 1) MG_LAUNCH(k_sleep_pass<1>, grid, dim3(64), 0, s, A);
    else if (lanes == 16) MG_LAUNCH(k_sleep_pass<16>, grid, dim3(64), 0, s, A);
    else if (lanes == 64) MG_LAUNCH(k_sleep_pass<64>, grid, dim3(64), 0, s, A);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t mg_launch_wake(const int* idx, int n, const int* table, int n_table, int n_island, int* timer, int* asleep,
                          hipStream_t s) {
    if (n <= 0 || n_island <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_wake_actors, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, idx, n, table, n_table, n_island, timer, asleep);
    return hipGetLastError();
}

hipError_t mg_launch_wake_ext(const float* ext, int nb, const int* body_island, int* timer, int* asleep, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_wake_ext, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, s, ext, nb, body_island, timer, asleep);
    return hipGetLastError();
}

hipError_t mg_launch_sleep_actors(const int* actor_island, int na, const int* asleep, int* dst, hipStream_t s) {
    if (na <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sleep_actors, dim3((unsigned)((na + 63) / 64)), dim3(64), 0, s, actor_island, na, asleep, dst);
    return hipGetLastError();
}

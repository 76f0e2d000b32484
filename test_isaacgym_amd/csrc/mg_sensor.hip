// mg_sensor.hip — force sensors: the joint reaction on an
// articulation's body by momentum balance over the frame, from what the step
// kernels already write (body states, applied wrenches, net contact forces)
// and the contact moments k_env_step's SENS builds keep.
//
//   k_sensor_mark   before the step: did the frame begin with a state set?
//   k_force_sensor  after the step: one lane per sensor
//
// Numerics of §3.4: -ffp-contract=off, every sum in a fixed order (the subtree
// in link order), no library transcendental.
#include "mg_internal.h"
#include "mg_math.h"

namespace {

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_int(a) == __float_as_int(b); }

// One lane per articulation that carries a sensor: compares the copy of its
// root row and DOF rows kept at the end of the last frame (k_force_sensor) bit
// by bit with the arrays now. A difference means a set_dof_state / root set
// came between: the link rows are stale, the frame's start state is unknown and
// the articulation's sensors read 0 this frame. So does the first frame (no
// copy yet). Lane 0 also turns the momentum history's halves over.
__global__ void __launch_bounds__(64) k_sensor_mark(MgSensorArgs A) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a == 0) *A.parity = *A.parity ^ 1;
    if (a >= A.n_art) return;
    const int* r = A.sart_i + (size_t)a * MG_SART_I_N;
    const int slot = r[0], d0 = r[1], nd = r[2];
    const float* sv = A.save + r[3];
    bool diff = A.valid[a] == 0;
    for (int f = 0; f < MG_STATE_N; ++f) diff = diff || !same_bits(sv[f], A.state[(size_t)f * A.nb + slot]);
    for (int d = 0; d < nd; ++d) {
        diff = diff || !same_bits(sv[MG_STATE_N + 2 * d], A.dof[d0 + d]);
        diff = diff || !same_bits(sv[MG_STATE_N + 2 * d + 1], A.dof[(size_t)A.nd + d0 + d]);
    }
    A.mark[a] = diff ? 1 : 0;
}

// One lane per sensor. Walks the links of the sensor body's subtree in link
// order; per body k: the end-of-frame momentum (m v+, I_w+ w+) (written to this
// frame's half of the history, last frame's read from the other), the frame's
// net wrench N_k, and (F_k, T_k) = N_k - G_k - E_k - C_k moved to the sensor
// origin. The forward-dynamics part (N - G - E) and the constraint part (-C)
// are summed apart, turned into the sensor frame apart and added once at the
// end, so the two parts read alone sum to the whole but for that one addition.
__global__ void __launch_bounds__(64) k_force_sensor(MgSensorArgs A) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= A.n) return;
    const int n = A.n, nb = A.nb, nhb = A.nhb;
    const int g0 = A.sens_i[MG_SENS_I_G0 * n + t];
    const int* li = A.link_i + (size_t)A.sens_i[MG_SENS_I_LINK0 * n + t] * MG_LINK_I_N;
    const int ls = A.sens_i[MG_SENS_I_LINK * n + t];
    unsigned mask = (unsigned)A.sens_i[MG_SENS_I_MASK * n + t];
    const int flags = A.sens_i[MG_SENS_I_FLAGS * n + t];
    const int art = A.sens_i[MG_SENS_I_ART * n + t];
    const int hb0 = A.sens_i[MG_SENS_I_HIST * n + t];
    const int par = *A.parity;
    float* hc = A.hist + (size_t)par * 6 * nhb;
    const float* hp = A.hist + (size_t)(par ^ 1) * 6 * nhb;
    const float* St = A.state;
    const float* Ms = A.mass;
    const V3 gv = v3(A.g[0], A.g[1], A.g[2]);

    // the sensor frame at the end of the frame
    const int bs = A.perm[g0 + li[ls * MG_LINK_I_N + 3]];
    const V3 xs = v3(St[0 * nb + bs], St[1 * nb + bs], St[2 * nb + bs]);
    const Q4 qs = q4(St[3 * nb + bs], St[4 * nb + bs], St[5 * nb + bs], St[6 * nb + bs]);
    const V3 pl = v3(A.sens_f[0 * n + t], A.sens_f[1 * n + t], A.sens_f[2 * n + t]);
    const Q4 ql = q4(A.sens_f[3 * n + t], A.sens_f[4 * n + t], A.sens_f[5 * n + t], A.sens_f[6 * n + t]);
    const V3 os = vadd(xs, qrot(qs, pl));

    V3 Ff = v3(0.0f, 0.0f, 0.0f), Tf = Ff, Fc = Ff, Tc = Ff;
    while (mask) {
        const int l = __ffs(mask) - 1;
        mask &= mask - 1;
        const int j = li[l * MG_LINK_I_N + 3];
        if (j < 0) continue;                       // a virtual link: no body row
        const int b = A.perm[g0 + j];
        const V3 x = v3(St[0 * nb + b], St[1 * nb + b], St[2 * nb + b]);
        const Q4 q = q4(St[3 * nb + b], St[4 * nb + b], St[5 * nb + b], St[6 * nb + b]);
        const V3 v = v3(St[7 * nb + b], St[8 * nb + b], St[9 * nb + b]);
        const V3 w = v3(St[10 * nb + b], St[11 * nb + b], St[12 * nb + b]);
        const float ix = Ms[1 * nb + b], iy = Ms[2 * nb + b], iz = Ms[3 * nb + b];
        const V3 Id = v3(ix > 0.0f ? 1.0f / ix : 0.0f, iy > 0.0f ? 1.0f / iy : 0.0f, iz > 0.0f ? 1.0f / iz : 0.0f);
        const Q4 iq = q4(Ms[4 * nb + b], Ms[5 * nb + b], Ms[6 * nb + b], Ms[7 * nb + b]);
        const V3 com = v3(Ms[8 * nb + b], Ms[9 * nb + b], Ms[10 * nb + b]);
        const float m = Ms[11 * nb + b];
        const float gon = A.tbf[A.body_tmpl[b] * MG_TBODY_F_N + 4];
        // momentum at the end of the frame: m v, R diag(I_p) R^T w
        const V3 pm = vscale(v, m);
        const M3 Rp = qmat(qmul(q, iq));
        const V3 wp = mtmul(Rp, w);
        const V3 lm = mmul(Rp, v3(Id.x * wp.x, Id.y * wp.y, Id.z * wp.z));
        const int hb = hb0 + j;
        const V3 pm0 = v3(hp[0 * nhb + hb], hp[1 * nhb + hb], hp[2 * nhb + hb]);
        const V3 lm0 = v3(hp[3 * nhb + hb], hp[4 * nhb + hb], hp[5 * nhb + hb]);
        hc[0 * nhb + hb] = pm.x; hc[1 * nhb + hb] = pm.y; hc[2 * nhb + hb] = pm.z;
        hc[3 * nhb + hb] = lm.x; hc[4 * nhb + hb] = lm.y; hc[5 * nhb + hb] = lm.z;
        // (F, T) = N - G - E about the body's COM
        V3 F = vscale(vsub(pm, pm0), A.inv_dt);
        V3 T = vscale(vsub(lm, lm0), A.inv_dt);
        if (gon != 0.0f) F = vsub(F, vscale(gv, m));
        F = vsub(F, v3(A.ext[0 * nb + b], A.ext[1 * nb + b], A.ext[2 * nb + b]));
        T = vsub(T, v3(A.ext[3 * nb + b], A.ext[4 * nb + b], A.ext[5 * nb + b]));
        const V3 Cf = v3(A.cforce[0 * nb + b], A.cforce[1 * nb + b], A.cforce[2 * nb + b]);
        const V3 Ct = v3(A.ctorque[0 * nb + b], A.ctorque[1 * nb + b], A.ctorque[2 * nb + b]);
        // to the sensor origin
        const V3 r = vsub(vadd(x, qrot(q, com)), os);
        Ff = vadd(Ff, F);
        Tf = vadd(Tf, vadd(T, vcross(r, F)));
        Fc = vsub(Fc, Cf);
        Tc = vsub(Tc, vadd(Ct, vcross(r, Cf)));
    }
    const bool fd = (flags & MG_SENSOR_FORWARD) != 0, cs = (flags & MG_SENSOR_CONSTRAINT) != 0;
    // each part into the sensor frame, then their sum: a sensor of one part
    // reads that term bit for bit
    if (!(flags & MG_SENSOR_WORLD)) {
        const Q4 qw = qconj(qmul(qs, ql));
        Ff = qrot(qw, Ff); Tf = qrot(qw, Tf);
        Fc = qrot(qw, Fc); Tc = qrot(qw, Tc);
    }
    V3 F = v3(0.0f, 0.0f, 0.0f), T = F;
    if (fd) { F = Ff; T = Tf; }
    if (cs) { F = fd ? vadd(Ff, Fc) : Fc; T = fd ? vadd(Tf, Tc) : Tc; }
    if (A.mark[art] != 0) { F = v3(0.0f, 0.0f, 0.0f); T = F; }
    float* o = A.out + (size_t)A.sens_i[MG_SENS_I_OUT * n + t] * 6;
    o[0] = F.x; o[1] = F.y; o[2] = F.z;
    o[3] = T.x; o[4] = T.y; o[5] = T.z;

    // the articulation's state as this frame leaves it (k_sensor_mark's copy)
    if (A.sens_i[MG_SENS_I_OWNER * n + t] != 0) {
        const int* r = A.sart_i + (size_t)art * MG_SART_I_N;
        const int slot = r[0], d0 = r[1], nd = r[2];
        float* sv = A.save + r[3];
        for (int f = 0; f < MG_STATE_N; ++f) sv[f] = St[(size_t)f * nb + slot];
        for (int d = 0; d < nd; ++d) {
            sv[MG_STATE_N + 2 * d] = A.dof[d0 + d];
            sv[MG_STATE_N + 2 * d + 1] = A.dof[(size_t)A.nd + d0 + d];
        }
        A.valid[art] = 1;
    }
}

}  // namespace

hipError_t mg_launch_sensor_mark(const MgSensorArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    MG_LAUNCH(k_sensor_mark, dim3((A.n_art + 63) / 64), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t mg_launch_force_sensor(const MgSensorArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    MG_LAUNCH(k_force_sensor, dim3((A.n + 63) / 64), dim3(64), 0, s, A);
    return hipGetLastError();
}

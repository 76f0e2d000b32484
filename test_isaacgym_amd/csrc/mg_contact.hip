// mg_contact.hip — the rigid contact list: packs the staging
// records the reporting builds of the step kernels left (mg_contact.h) into one
// device-resident list of mg_rigid_contact records.
//
// Owners are numbered family by family (free bodies by storage slot, coupled
// envs, pile envs); owner o's entries go to base(o) + k, base the exclusive
// prefix sum of the owners' entry counts. The sum is taken within a block of
// MG_CREP_BLOCK owners and then across blocks, in two small passes:
//   k_contact_count    block b's entry total -> blk_sum[b]
//   k_contact_compact  base of block b = sum of blk_sum[0..b) (every block adds
//                      them itself: at most a few thousand ints out of L2), an
//                      exclusive scan of its owners' counts in LDS, then each
//                      lane copies its owner's entries, adding the env index
//                      (the staging reads coalesced over a wave's owners).
// Both are plain launches on the step's stream (capturable). The list's order
// is deterministic: owner order, then the kernel's own contact order. Entries
// past `capacity` are dropped, never written; the header keeps both totals.
#include "mg_internal.h"

namespace {

struct Owner {
    int f, i;   // family, index within it (f == MG_CREP_FAMILIES: none)
    int c;      // its index in the family's stage / count arrays
};
__device__ __forceinline__ Owner owner_of(const MgContactArgs& A, int o) {
    Owner w{0, o, 0};
#pragma unroll
    for (int f = 0; f < MG_CREP_FAMILIES; ++f) {
        if (w.f == f && w.i >= A.fam[f].n) {
            w.i -= A.fam[f].n;
            w.f = f + 1;
        }
    }
    return w;
}
// the family's record as scalars (a dynamic index into the argument block would
// go through scratch)
__device__ __forceinline__ MgContactFamily family(const MgContactArgs& A, int f) {
    static_assert(MG_CREP_FAMILIES == 3, "family(): one select per family");
#define MG_FAM_SEL(x) (f == 0 ? A.fam[0].x : (f == 1 ? A.fam[1].x : A.fam[2].x))
    MgContactFamily F;
    F.n = MG_FAM_SEL(n);
    F.cap = MG_FAM_SEL(cap);
    F.stride = MG_FAM_SEL(stride);
    F.stage = MG_FAM_SEL(stage);
    F.count = MG_FAM_SEL(count);
    F.env = MG_FAM_SEL(env);
    F.col = MG_FAM_SEL(col);
#undef MG_FAM_SEL
    return F;
}
// entries of owner o (0 past the last owner), clamped to the record's capacity
__device__ __forceinline__ int owner_count(const MgContactArgs& A, int o, Owner& w, MgContactFamily& F) {
    w = owner_of(A, o);
    if (o >= A.n_own || w.f >= MG_CREP_FAMILIES) {
        w.f = MG_CREP_FAMILIES;
        return 0;
    }
    F = family(A, w.f);
    w.c = F.col ? F.col[w.i] : w.i;
    return min(max(F.count[w.c], 0), F.cap);
}
__device__ __forceinline__ int block_sum(int v, int* lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = MG_CREP_BLOCK / 2; d > 0; d >>= 1) {
        if (t < d) lds[t] += lds[t + d];
        __syncthreads();
    }
    const int r = lds[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(MG_CREP_BLOCK) k_contact_count(MgContactArgs A) {
    __shared__ int lds[MG_CREP_BLOCK];
    Owner w;
    MgContactFamily F;
    const int c = owner_count(A, blockIdx.x * MG_CREP_BLOCK + threadIdx.x, w, F);
    const int sum = block_sum(c, lds);
    if (threadIdx.x == 0) A.blk_sum[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(MG_CREP_BLOCK) k_contact_compact(MgContactArgs A) {
    __shared__ int lds[MG_CREP_BLOCK];
    const int t = threadIdx.x;
    // this block's base: the totals of the blocks before it
    int part = 0;
    for (int b = t; b < (int)blockIdx.x; b += MG_CREP_BLOCK) part += A.blk_sum[b];
    const int base0 = block_sum(part, lds);
    Owner w;
    MgContactFamily F;
    const int c = owner_count(A, blockIdx.x * MG_CREP_BLOCK + t, w, F);
    // inclusive scan of the block's counts (Hillis-Steele in LDS)
    lds[t] = c;
    __syncthreads();
    for (int d = 1; d < MG_CREP_BLOCK; d <<= 1) {
        const int add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int base = base0 + lds[t] - c;
    if (blockIdx.x == gridDim.x - 1 && t == MG_CREP_BLOCK - 1) {
        const int total = base0 + lds[t];
        const int stored = min(total, A.capacity);
        A.header[0] = total;
        A.header[1] = stored;
        A.header_host[0] = total;
        A.header_host[1] = stored;
    }
    if (c == 0) return;
    // one lane per owner, entry by entry: the staging reads of a wave are then
    // coalesced over the owners (the staging is owner-minor), each entry four
    // 16-byte stores. A wave per env with lane = (entry, quarter) makes the
    // stores one contiguous run but its reads single dwords a stride apart: it
    // measured slower (4096 30-ball piles: 215 us per simulate against 162 us).
    const int env = F.env[w.i];
    const size_t s = (size_t)F.stride;
    for (int k = 0; k < c; ++k) {
        const int at = base + k;
        if (at >= A.capacity) break;   // dropped, never written
        const float* e = F.stage + (size_t)k * MG_CREP_N * s + w.c;
        float4* o = reinterpret_cast<float4*>(A.out + at);
        o[0] = make_float4(__int_as_float(env), e[0 * s], e[1 * s], e[2 * s]);
        o[1] = make_float4(e[4 * s], e[5 * s], e[6 * s], e[7 * s]);
        o[2] = make_float4(e[8 * s], e[9 * s], e[10 * s], e[11 * s]);
        o[3] = make_float4(e[12 * s], e[13 * s], e[14 * s], e[15 * s]);
    }
}

}  // namespace

hipError_t mg_launch_contact_compact(const MgContactArgs& A, hipStream_t s) {
    if (A.n_own <= 0 || A.nblk <= 0) return hipSuccess;
    MG_LAUNCH(k_contact_count, dim3(A.nblk), dim3(MG_CREP_BLOCK), 0, s, A);
    MG_LAUNCH(k_contact_compact, dim3(A.nblk), dim3(MG_CREP_BLOCK), 0, s, A);
    return hipGetLastError();
}

// The frame shared by the RANSAC solvers that take K independent problems per call (sim3.hip, mlpnp.hip): each problem has N
// correspondences and `iters` minimal sets drawn by the caller, every hypothesis is counted by one wavefront, and one workgroup per
// problem applies the solver's result rule.  What a solver adds is its own fields, kernels, predicate and rule.
#pragma once

namespace eorb {

// the part of a problem that the frame reads; corr_off / set_off: where its correspondences / sets begin in the flat arrays
struct RansacProb { int N, iters, corr_off, set_off, min_inliers; };

// the head of a solver's argument block: its problems (device memory; Prob begins with a RansacProb) and the launch extents
template <class Prob> struct RansacSet { const Prob* prob; int K, max_N, max_iters; };

// a problem with fewer correspondences than min_inliers runs no iteration; its finish kernel writes the solver's record for that case
__device__ __forceinline__ bool ransac_skips(const RansacProb& P) { return P.N < P.min_inliers; }

// how many of the correspondences 0 .. N-1 satisfy pred(i), by one wavefront: lane l takes l, l + 64, ...; every lane returns the count.
// A lane past N does not evaluate pred.
template <class Pred> __device__ __forceinline__ int ransac_count_inliers(int N, Pred pred)
{
    const int lane = threadIdx.x;
    int n = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool in = i < N && pred(i);
        n += __popcll(__ballot(in));
    }
    return n;
}

}  // namespace eorb

// rl_train_population.hip — the population kernels (rl.h rl_population_create): one
// launch steps M independent shared-Q agents, workgroup m = member m.  The step loop
// is train_shared_body's (rl_train_impl.h, POP = true): the generic family only (no
// recording, the episodic bookkeeping by KParams::episodic), one-step agents, in f64
// and — where the range proof can hold (fix_possible) — in the fixed point.
#include "rl_train_impl.h"

namespace rlamd {

// The block's member: its table rows and its scalars replace the handle-wide ones in
// the block's copy of the parameter block, so the body reads them where a lone agent's
// kernel reads its own.  blockIdx.x is uniform, so the member's record comes in by
// scalar loads before the step loop and the scalars stay in SGPRs like kernel
// arguments.  Offsets are 64-bit (M * P*S*A words may pass 2^32 bytes).
template <int ENV, int POLICY, int SEL, int ALGO, bool FQ>
__global__ void __launch_bounds__(1024) k_train_population(KParams p, PopParams pp) {
    const uint64_t m = blockIdx.x;
    const uint64_t SA = (uint64_t)p.S * p.A;
    const MemberParams mp = pp.members[m];
    p.q_base = pp.q + m * ((uint64_t)p.P * SA);
    p.n_base = pp.n + m * SA;
    p.t_base = pp.t + m;
    p.lr = mp.lr;
    p.lr40 = mp.lr40;
    p.gamma = mp.gamma;
    p.eps_dm = mp.eps_dm;
    p.eps_ds = mp.eps_ds;
    p.eps_final = mp.eps_final;
    p.ucb_c = mp.ucb_c;
    train_shared_body<ENV, RL_AGENT_ONE_STEP, POLICY, SEL, ALGO, false, FQ, -1, -1, false, -1, -1, true>(
        p, pp.stats + m * STATS_W);
}

template <int ENV, int POLICY, int SEL, int ALGO>
hipError_t launch_population(const KParams &p, const PopParams &pp, dim3 grid, dim3 block, size_t smem,
                             hipStream_t stream, int *occ) {
    const void *k = nullptr;
    if (p.fq) k = (const void *)k_train_population<ENV, POLICY, SEL, ALGO, true>;
    else if constexpr (fix_possible<RL_AGENT_ONE_STEP, POLICY, SEL, ALGO>())
        k = (const void *)k_train_population<ENV, POLICY, SEL, ALGO, false>;
    if (!k) return hipErrorInvalidValue;   // the fixed point for a variant it cannot prove
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    if (occ) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k, (int)(block.x * block.y * block.z), smem);
    void *args[] = {(void *)&p, (void *)&pp};
    return hipLaunchKernel(k, grid, block, args, smem, stream);
}

template <int ENV>
pop_launch_fn population_entry(int policy, int sel, int algo) {
#define RLAMD_P(PO, SE, AL)                                                                        \
    if (policy == PO && sel == SE && algo == AL) return &launch_population<ENV, PO, SE, AL>;
#define RLAMD_P1(PO)                                                                               \
    RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_SARSA) RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_QLEARNING) \
    RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_EXPECTED_SARSA) RLAMD_P(PO, RL_SEL_UCB, RL_ALGO_SARSA)   \
    RLAMD_P(PO, RL_SEL_UCB, RL_ALGO_QLEARNING)
    RLAMD_P1(RL_POLICY_TABULAR)
    RLAMD_P1(RL_POLICY_DOUBLE)
#undef RLAMD_P1
#undef RLAMD_P
    return nullptr;   // UCB + expected SARSA: preset counters and their layout, not in a population yet
}

pop_launch_fn lookup_population(int env, int policy, int sel, int algo) {
    switch (env) {
    case RL_ENV_FROZEN_LAKE: return population_entry<RL_ENV_FROZEN_LAKE>(policy, sel, algo);
    case RL_ENV_CLIFF_WALKING: return population_entry<RL_ENV_CLIFF_WALKING>(policy, sel, algo);
    case RL_ENV_TAXI: return population_entry<RL_ENV_TAXI>(policy, sel, algo);
    case RL_ENV_BLACKJACK: return population_entry<RL_ENV_BLACKJACK>(policy, sel, algo);
    }
    return nullptr;
}

}  // namespace rlamd

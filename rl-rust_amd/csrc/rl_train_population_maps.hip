// rl_train_population_maps.hip — the population kernels on maps of the members' own
// (rl.h rl_population_create_maps): k_train_population's launch (rl_train_population.hip;
// workgroup m = member m, train_shared_body with POP = true) over the registered-map
// envs, where member m also brings its own transition table and start rule.
#include "rl_train_impl.h"

namespace rlamd {

// The block's member, as k_train_population takes it, and the member's env: its
// transition table, start list, n_start and fixed_start replace the handle-wide ones
// in the block's copy of the parameter block.  blockIdx.x is uniform, so both records
// come in by scalar loads before the step loop.  The LDS carve is the population's
// (pm.carve_n_start, the largest start list): the same in every block, whatever the
// member's own n_start, which drives only its list's copy and search.  A member with
// a fixed start has n_start 0: it copies nothing and never reads `start`.
template <int ENV, int POLICY, int SEL, int ALGO, bool FQ>
__global__ void __launch_bounds__(1024) k_train_population_maps(KParams p, PopParams pp, PopMapParams pm) {
    static_assert(env_map_start(ENV), "the members' own maps run the registered-map envs");
    const uint64_t m = blockIdx.x;
    const uint64_t SA = (uint64_t)p.S * p.A;
    const MemberParams mp = pp.members[m];
    const MemberEnv me = pm.envs[m];
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
    p.trans = me.trans;
    p.start_cdf = me.start;
    p.n_start = me.n_start;
    p.fixed_start = me.fixed_start;
    train_shared_body<ENV, RL_AGENT_ONE_STEP, POLICY, SEL, ALGO, false, FQ, -1, -1, false, -1, -1, true>(
        p, pp.stats + m * STATS_W, pm.carve_n_start);
}

template <int ENV, int POLICY, int SEL, int ALGO>
hipError_t launch_population_maps(const KParams &p, const PopParams &pp, const PopMapParams &pm, dim3 grid,
                                  dim3 block, size_t smem, hipStream_t stream, int *occ) {
    const void *k = nullptr;
    if (p.fq) k = (const void *)k_train_population_maps<ENV, POLICY, SEL, ALGO, true>;
    else if constexpr (fix_possible<RL_AGENT_ONE_STEP, POLICY, SEL, ALGO>())
        k = (const void *)k_train_population_maps<ENV, POLICY, SEL, ALGO, false>;
    if (!k) return hipErrorInvalidValue;   // the fixed point for a variant it cannot prove
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    if (occ) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k, (int)(block.x * block.y * block.z), smem);
    void *args[] = {(void *)&p, (void *)&pp, (void *)&pm};
    return hipLaunchKernel(k, grid, block, args, smem, stream);
}

template <int ENV>
pop_maps_launch_fn population_maps_entry(int policy, int sel, int algo) {
#define RLAMD_P(PO, SE, AL)                                                                        \
    if (policy == PO && sel == SE && algo == AL) return &launch_population_maps<ENV, PO, SE, AL>;
#define RLAMD_P1(PO)                                                                               \
    RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_SARSA) RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_QLEARNING) \
    RLAMD_P(PO, RL_SEL_EPS_GREEDY, RL_ALGO_EXPECTED_SARSA) RLAMD_P(PO, RL_SEL_UCB, RL_ALGO_SARSA)   \
    RLAMD_P(PO, RL_SEL_UCB, RL_ALGO_QLEARNING)
    RLAMD_P1(RL_POLICY_TABULAR)
    RLAMD_P1(RL_POLICY_DOUBLE)
#undef RLAMD_P1
#undef RLAMD_P
    return nullptr;   // UCB + expected SARSA: not in a population (rl_train_population.hip)
}

pop_maps_launch_fn lookup_population_maps(int env, int policy, int sel, int algo) {
    switch (env) {
    case ENV_FL_MAP: return population_maps_entry<ENV_FL_MAP>(policy, sel, algo);
    case ENV_FLE_MAP: return population_maps_entry<ENV_FLE_MAP>(policy, sel, algo);
    case ENV_FL_WIDE: return population_maps_entry<ENV_FL_WIDE>(policy, sel, algo);
    case ENV_FLE_WIDE: return population_maps_entry<ENV_FLE_WIDE>(policy, sel, algo);
    }
    return nullptr;
}

}  // namespace rlamd

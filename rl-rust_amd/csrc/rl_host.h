// rl_host.h — what the host runtime's two files share: rl_host_env.cpp builds the
// env tables on the host (no HIP runtime call), rl_host.cpp owns the handles, the
// device memory and the launches.  Private to the library: nothing here is exported.
#pragma once
#include <string>
#include <vector>

#include "rl_kparams.h"

#pragma GCC visibility push(hidden)

// the calling thread's rl_last_error text; returns `code`
int fail(int code, const std::string &msg);

// The product's own construction of the reference envs (an independent
// restatement from the oracle's and from tests/golden/make_tables.py).
struct EnvHost {
    int kind = 0;
    uint32_t S = 0, A = 0, max_steps = 0;
    std::vector<uint32_t> trans;  // packed, see rl_device.h EnvDev<>
    std::vector<double> start;    // initial-state distribution
    std::vector<double> cdf;      // running sum of `start` (categorical_sample, utils.rs:33-43)
    double th1 = 0, th2 = 0, th3 = 0, trunc_reward = 0;
    int32_t fixed_start = -1;     // categorical_sample over `cdf` is constant (single start state)
    int32_t slippery = 0;         // FrozenLake with stochastic rows
    std::vector<std::string> map;   // FrozenLake / FrozenLakeEdited grid (nrow x ncol); empty otherwise
    int nrow = 0, ncol = 0;
    int kenv = 0;                 // kernel-side env id (rl_kparams.h): kind, or ENV_FL_MAP / ENV_FLE_MAP
    // registered maps with two or more 'S' cells: the start list the device searches,
    // [n_list f64 running sums][n_list u32 cells] packed in f64 words (rl_kparams.h)
    std::vector<double> start_list;
    uint32_t n_list = 0;
    // what the device reads as KParams::start_cdf / n_start
    const std::vector<double> &dev_cdf() const { return rlamd::env_map_start(kenv) ? start_list : cdf; }
    uint32_t dev_n_start() const { return rlamd::env_map_start(kenv) ? n_list : (uint32_t)cdf.size(); }
};

// as_map: a built-in FrozenLake map (id 0 / 1) in the registered maps' form too
// (ENV_FL_MAP / ENV_FLE_MAP, fixed_start 0)
int build_env(const rl_env_config &c, EnvHost &e, bool as_map = false);
int net_feature_table(const rl_env_config &c, const EnvHost &e, int input, std::vector<double> &feat, uint32_t &n_in);

#pragma GCC visibility pop

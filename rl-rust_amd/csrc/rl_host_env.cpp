// rl_host_env.cpp — the host runtime's env tables (rl_host.h): the reference envs'
// transition tables and start distributions, the FrozenLake map registry, and the
// calls of include/rl.h that need nothing else (rl_map_*, rl_env_dims,
// rl_env_table, rl_obs_*).  Host arithmetic only: no HIP runtime call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "rl_host.h"
#include "rl_taxi.h"

using namespace rlamd;

namespace {

// ------------------------------------------------------------------ env tables

const char *const kFL4[] = {"SFFF", "FHFH", "FFFH", "HFFG"};                     // frozen_lake.rs:23
const char *const kFL8[] = {"SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF",       // frozen_lake.rs:25-28
                            "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG"};
const char *const kTaxiMap[] = {"+---------+", "|R: | : :G|", "| : | : : |", "| : : : : |",
                                "| | : | : |", "|Y| : |B: |", "+---------+"};   // taxi.rs:22-30
const int kTaxiLocs[4][2] = {{0, 0}, {0, 4}, {4, 0}, {4, 3}};                   // taxi.rs:31

// utils::inc (src/utils.rs:53-76): 0 LEFT, 1 DOWN, 2 RIGHT, 3 UP, clamped
void grid_move(int nrow, int ncol, int row, int col, int a, int &nr, int &nc) {
    nr = row;
    nc = col;
    switch (a) {
    case 0: nc = std::max(col - 1, 0); break;
    case 1: nr = std::min(row + 1, nrow - 1); break;
    case 2: nc = std::min(col + 1, ncol - 1); break;
    case 3: nr = std::max(row - 1, 0); break;
    default: break;
    }
}

// FrozenLakeTerrain of a cell / of the neighbour in direction a, WALL off the
// grid (src/env/frozen_lake_edited.rs get_obs :115-144, get_terrain :146-162)
enum { kStart = 0, kWall = 1, kHole = 2, kGround = 3, kGoal = 4 };
using Grid = std::vector<std::string>;
int terrain(const Grid &map, int row, int col) {
    const char ch = map[row][col];
    return ch == 'S' ? kStart : ch == 'G' ? kGoal : ch == 'H' ? kHole : kGround;
}
int neighbour(const Grid &map, int nrow, int ncol, int row, int col, int a) {
    switch (a) {
    case 0: return col == 0 ? kWall : terrain(map, row, col - 1);
    case 1: return row == nrow - 1 ? kWall : terrain(map, row + 1, col);
    case 2: return col == ncol - 1 ? kWall : terrain(map, row, col + 1);
    default: return row == 0 ? kWall : terrain(map, row - 1, col);
    }
}
double terrain_value(int t) {   // FrozenLakeTerrain::value (frozen_lake_edited.rs:18-28)
    return t == kHole ? -1.0 : t == kWall ? -0.5 : t == kStart ? 0.0 : t == kGround ? 0.5 : 1.0;
}

void finish_cdf(EnvHost &e) {
    e.cdf.resize(e.start.size());
    double b = 0.0;
    for (size_t i = 0; i < e.start.size(); ++i) {
        b += e.start[i];
        e.cdf[i] = b;
    }
    // first i with cdf[i] > u for every u in [0, 1 - 2^-52]: fixed when all
    // earlier sums are 0 and cdf[i] exceeds the largest uniform
    e.fixed_start = -1;
    for (size_t i = 0; i < e.cdf.size(); ++i) {
        if (e.cdf[i] == 0.0) continue;
        if (e.cdf[i] > 1.0 - 0x1p-52) e.fixed_start = (int32_t)i;
        break;
    }
}

// categorical_sample over the cdf (utils.rs:33-43): first i with cdf[i] > u, else 0
uint32_t linear_sample(const std::vector<double> &cdf, double u) {
    for (size_t i = 0; i < cdf.size(); ++i)
        if (cdf[i] > u) return (uint32_t)i;
    return 0;
}
// rl_taxi.h taxi_start (three probes) equals the linear search at every
// boundary: each c_k and its neighbours, and the u around each k/300 where the
// first probe moves (between boundaries both are constant).  Checked once.
bool taxi_start_checked(const EnvHost &e) {
    static int ok = -1;
    if (ok >= 0) return ok == 1;
    std::vector<double> us = {0.0, std::nextafter(1.0, 0.0)};
    auto around = [&](double x) {
        double lo = x, hi = x;
        for (int i = 0; i < 8; ++i) { lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, 1.0); us.push_back(lo); us.push_back(hi); }
        us.push_back(x);
    };
    for (double c : e.cdf) if (c > 0.0 && c < 1.0) around(c);
    for (int j = 1; j < 300; ++j) around((double)j / 300.0);
    ok = 1;
    for (double u : us)
        if (u >= 0.0 && u < 1.0 && taxi_start(e.cdf.data(), u) != linear_sample(e.cdf, u)) ok = 0;
    return ok == 1;
}

// The process-wide map registry (rl.h rl_map_register): ids 0 / 1 are MAP_4X4 /
// MAP_8X8, registered maps get 2, 3, ... in registration order and keep them for
// the life of the process (nothing is ever removed, so an id is never reused).
std::mutex g_map_mu;
std::vector<Grid> &map_registry() {
    static std::vector<Grid> maps = {Grid(kFL4, kFL4 + 4), Grid(kFL8, kFL8 + 8)};
    return maps;
}
// the table format of every id (rl_map_register_wide: 1), parallel to the registry
std::vector<uint8_t> &map_wide_flags() {
    static std::vector<uint8_t> wide = {0, 0};
    return wide;
}
bool map_lookup(int32_t id, Grid &out, bool *wide = nullptr) {
    std::lock_guard<std::mutex> lock(g_map_mu);
    const std::vector<Grid> &maps = map_registry();
    if (id < 0 || (size_t)id >= maps.size()) return false;
    out = maps[(size_t)id];
    if (wide) *wide = map_wide_flags()[(size_t)id] != 0;
    return true;
}

}  // namespace

int build_env(const rl_env_config &c, EnvHost &e, bool as_map) {
    e = EnvHost();
    e.kind = c.kind;
    e.kenv = c.kind;
    e.max_steps = c.max_steps;
    if (c.kind == RL_ENV_FROZEN_LAKE || c.kind == RL_ENV_FROZEN_LAKE_EDITED) {
        const bool edited = c.kind == RL_ENV_FROZEN_LAKE_EDITED;
        bool wide = false;
        if (!map_lookup(c.map8x8, e.map, &wide))
            return fail(RL_E_ARG, "unknown FrozenLake map id " + std::to_string(c.map8x8) +
                                      " (0 = MAP_4X4, 1 = MAP_8X8, else an id from rl_map_register)");
        const Grid &map = e.map;
        // nrow x ncol, state = row * ncol + col (frozen_lake.rs:49-50, utils.rs:45-51)
        const int nrow = (int)map.size(), ncol = (int)map[0].size();
        e.nrow = nrow;
        e.ncol = ncol;
        // a registered map runs the kernels with the start variant (rl_kparams.h), a
        // built-in one exactly the instantiations it always ran — unless the caller asks
        // for the map form (as_map: a population on the members' own maps, where ids 0 / 1
        // are narrow maps with the fixed start 0)
        if (c.map8x8 >= 2 || as_map) e.kenv = edited ? ENV_FLE_MAP : ENV_FL_MAP;
        if (wide) e.kenv = edited ? ENV_FLE_WIDE : ENV_FL_WIDE;   // rl_map_register_wide: the wide table
        e.S = (uint32_t)(nrow * ncol);
        e.A = 4;
        e.trans.assign(e.S * 4, 0);
        int n_start = 0;
        for (int i = 0; i < nrow * ncol; ++i) n_start += map[i / ncol][i % ncol] == 'S';
        e.start.assign(e.S, 0.0);   // frozen_lake.rs:52-65: 1/k on each of the k 'S' cells
        for (int i = 0; i < nrow * ncol; ++i)
            if (map[i / ncol][i % ncol] == 'S') e.start[i] = 1.0 / n_start;
        // the deterministic outcome of direction a: next state, reward bit, terminated
        auto judge = [&](int row, int col, int a, uint32_t &ns, bool &goal, bool &done) {
            int nr, nc;
            grid_move(nrow, ncol, row, col, a, nr, nc);
            ns = (uint32_t)(nr * ncol + nc);
            if (edited) {   // update_probability_matrix (frozen_lake_edited.rs:94-113): judged by
                            // the terrain in the moved direction; 10.0 onto G, else -1.0
                const int t = neighbour(map, nrow, ncol, row, col, a);
                goal = t == kGoal;
                done = t == kGoal || t == kHole;
            } else {
                const char ch = map[nr][nc];
                goal = ch == 'G';
                done = ch == 'G' || ch == 'H';
            }
        };
        auto outcome = [&](int row, int col, int a) -> uint32_t {   // the packed byte (<= 64 cells)
            uint32_t ns;
            bool goal, done;
            judge(row, col, a, ns, goal, done);
            return ns | (goal ? 64u : 0u) | (done ? 128u : 0u);
        };
        for (int row = 0; !wide && row < nrow; ++row)
            for (int col = 0; col < ncol; ++col)
                for (int a = 0; a < 4; ++a) {
                    const int s = row * ncol + col;
                    const char ch = map[row][col];
                    uint32_t w;
                    if (ch == 'G' || ch == 'H') w = (uint32_t)s | 128u;              // (1.0, s, 0, true)
                    else if (c.slippery)                                             // [(a-1)%4, a, (a+1)%4]
                        w = outcome(row, col, (a + 3) & 3) | (outcome(row, col, a) << 8) |
                            (outcome(row, col, (a + 1) & 3) << 16) | (1u << 24);
                    else w = outcome(row, col, a);
                    e.trans[s * 4 + a] = w;
                }
        if (wide) {
            // the wide table (rl_kparams.h): one u16 per (s, direction), two per u32
            // word; 'G' / 'H' cells (s, 0, terminated) in every direction
            std::vector<uint16_t> t16((size_t)e.S * 4);
            for (int row = 0; row < nrow; ++row)
                for (int col = 0; col < ncol; ++col)
                    for (int d = 0; d < 4; ++d) {
                        const int s = row * ncol + col;
                        const char ch = map[row][col];
                        uint32_t ns;
                        bool goal, done;
                        judge(row, col, d, ns, goal, done);
                        t16[(size_t)s * 4 + d] =
                            (ch == 'G' || ch == 'H')
                                ? (uint16_t)((uint32_t)s | WIDE_TERM)
                                : (uint16_t)(ns | (goal ? WIDE_REWARD : 0u) | (done ? WIDE_TERM : 0u));
                    }
            e.trans.assign((size_t)e.S * 2, 0);
            std::memcpy(e.trans.data(), t16.data(), t16.size() * 2);
        }
        e.slippery = c.slippery ? 1 : 0;
        const double third = 1.0 / 3.0;
        e.th1 = 0.0 + third;
        e.th2 = e.th1 + third;
        e.th3 = e.th2 + third;
        e.trunc_reward = edited ? -1.0 : 0.0;   // frozen_lake.rs:119-122 / frozen_lake_edited.rs:227-231
    } else if (c.kind == RL_ENV_CLIFF_WALKING) {
        e.S = 48;
        e.A = 4;
        e.trans.assign(48 * 4, 0);
        for (int row = 0; row < 4; ++row)
            for (int col = 0; col < 12; ++col)
                for (int a = 0; a < 4; ++a) {
                    int nr, nc;
                    grid_move(4, 12, row, col, a, nr, nc);
                    const int ns = nr * 12 + nc;
                    const bool cliff = ns >= 37 && ns <= 46, goal = ns == 47;  // cliff_walking.rs:9-11
                    e.trans[(row * 12 + col) * 4 + a] =
                        (uint32_t)ns | (cliff ? 64u : 0u) | ((cliff || goal) ? 128u : 0u);
                }
        e.start.assign(48, 0.0);
        e.start[36] = 1.0;
        e.trunc_reward = -100.0;
    } else if (c.kind == RL_ENV_TAXI) {
        e.S = 500;
        e.A = 6;
        e.trans.assign(500 * 6, 0);
        e.start.assign(500, 0.0);
        double total = 0.0;
        auto enc = [](int r, int cc, int p, int d) { return ((r * 5 + cc) * 5 + p) * 4 + d; };
        for (int r = 0; r < 5; ++r)
            for (int cc = 0; cc < 5; ++cc)
                for (int p = 0; p < 5; ++p)
                    for (int d = 0; d < 4; ++d) {
                        const int s = enc(r, cc, p, d);
                        if (p < 4 && p != d) { e.start[s] += 1.0; total += 1.0; }
                        for (int a = 0; a < 6; ++a) {
                            int nr = r, nc = cc, np = p;
                            uint32_t rcode = 0;  // -1
                            bool term = false;
                            if (a == 0) nr = std::min(r + 1, 4);
                            else if (a == 1) nr = std::max(r - 1, 0);
                            if (a == 2 && kTaxiMap[1 + r][2 * cc + 2] == ':') nc = std::min(cc + 1, 4);
                            else if (a == 3 && kTaxiMap[1 + r][2 * cc] == ':') nc = std::max(cc - 1, 0);
                            else if (a == 4) {
                                if (p < 4 && r == kTaxiLocs[p][0] && cc == kTaxiLocs[p][1]) np = 4;
                                else rcode = 1;  // -10
                            } else if (a == 5) {
                                if (r == kTaxiLocs[d][0] && cc == kTaxiLocs[d][1] && p == 4) {
                                    np = d; term = true; rcode = 2;  // +20
                                } else rcode = 1;
                            }
                            e.trans[s * 6 + a] = (uint32_t)enc(nr, nc, np, d) | (rcode << 9) | ((term ? 1u : 0u) << 11);
                        }
                    }
        for (double &v : e.start) v /= total;   // taxi.rs:117-119
        e.trunc_reward = 0.0;
        // the kernels compute Taxi's transitions (rl_taxi.h taxi_word): all 3000 must
        // equal the table built above
        for (uint32_t i = 0; i < 500u * 6u; ++i)
            if (taxi_word(i / 6u, i % 6u) != e.trans[i]) return fail(RL_E_STATE, "taxi_word differs from the table");
    } else if (c.kind == RL_ENV_BLACKJACK) {
        e.S = 32 * 32 * 2;   // dense (p_score <= 31, d_score <= 26 in 5 bits, p_ace): (p*32 + d)*2 + ace
        e.A = 2;
    } else {
        return fail(RL_E_ARG, "unknown env kind");
    }
    if (!e.start.empty()) finish_cdf(e);
    if (c.kind == RL_ENV_TAXI && !taxi_start_checked(e)) return fail(RL_E_STATE, "taxi_start differs from categorical_sample");
    if (env_map_start(e.kenv)) {
        // Env::reset on a registered map (DESIGN §2 "draws"): no 'S' is the all-false
        // argmax's cell 0 (utils.rs:33-43), one 'S' a fixed start, neither drawn; two
        // or more draw one uniform01 and search the list of the 'S' cells with their
        // running sums — the sum changes nowhere else, so this is the full scan.
        std::vector<uint32_t> cells;
        for (uint32_t i = 0; i < e.S; ++i)
            if (e.start[i] != 0.0) cells.push_back(i);
        if (cells.empty()) e.fixed_start = 0;
        else if (cells.size() == 1) e.fixed_start = (int32_t)cells[0];
        else {
            e.fixed_start = -1;
            e.n_list = (uint32_t)cells.size();
            e.start_list.assign(e.n_list + (e.n_list + 1) / 2, 0.0);
            for (uint32_t j = 0; j < e.n_list; ++j) e.start_list[j] = e.cdf[cells[j]];
            std::memcpy(e.start_list.data() + e.n_list, cells.data(), cells.size() * sizeof(uint32_t));
            // the list against the full scan at every boundary and its neighbours
            std::vector<double> us = {0.0, std::nextafter(1.0, 0.0)};
            for (uint32_t j = 0; j < e.n_list; ++j)
                for (double x : {e.start_list[j], std::nextafter(e.start_list[j], 0.0), std::nextafter(e.start_list[j], 2.0)})
                    if (x >= 0.0 && x < 1.0) us.push_back(x);
            for (double u : us) {
                uint32_t got = 0;
                for (uint32_t j = 0; j < e.n_list; ++j)
                    if (e.start_list[j] > u) { got = cells[j]; break; }
                if (got != linear_sample(e.cdf, u)) return fail(RL_E_STATE, "start list differs from categorical_sample");
            }
        }
    } else if (!e.map.empty() && e.fixed_start != 0) {
        // the built-in maps' kernels reset to the constant 0 (rl_device.h)
        return fail(RL_E_STATE, "built-in FrozenLake map does not start at position 0");
    }
    return RL_OK;
}

// NeuralPolicy input features of every dense state (rl.h rl_input_adapter)
int net_feature_table(const rl_env_config &c, const EnvHost &e, int input, std::vector<double> &feat, uint32_t &n_in) {
    if (input == RL_INPUT_FL_OBS) {
        if (e.map.empty()) return fail(RL_E_ARG, "the FrozenLakeObs adapter needs FrozenLake / FrozenLakeEdited");
        n_in = 6;
        feat.assign((size_t)e.S * 6, 0.0);
        for (uint32_t s = 0; s < e.S; ++s) {
            const int row = (int)s / e.ncol, col = (int)s % e.ncol;   // x = row, y = col (frozen_lake_edited.rs:146-147)
            for (int a = 0; a < 4; ++a)
                feat[s * 6 + a] = terrain_value(neighbour(e.map, e.nrow, e.ncol, row, col, a));
            feat[s * 6 + 4] = (double)row;
            feat[s * 6 + 5] = (double)col;
        }
        return RL_OK;
    }
    if (input != RL_INPUT_SCALAR) return fail(RL_E_ARG, "unknown input adapter");
    if (c.kind == RL_ENV_FROZEN_LAKE_EDITED)
        return fail(RL_E_ARG, "FrozenLakeEdited observations are FrozenLakeObs structs: use RL_INPUT_FL_OBS");
    n_in = 1;
    feat.assign(e.S, 0.0);
    for (uint32_t s = 0; s < e.S; ++s) feat[s] = (double)rl_obs_to_reference(c.kind, s);   // obs as f64
    return RL_OK;
}

// ====================================================================== C ABI
extern "C" {

uint64_t rl_blackjack_obs_id(uint32_t p, uint32_t d, uint32_t ace) {
    // fxhash 0.2.1: FxHasher64::write_u8 per field of #[derive(Hash)]
    const uint64_t K = 0x517cc1b727220a95ull;
    uint64_t h = 0;
    const uint64_t w[3] = {p & 0xffu, d & 0xffu, ace ? 1u : 0u};
    for (uint64_t x : w) h = (((h << 5) | (h >> 59)) ^ x) * K;
    return h;
}
uint64_t rl_obs_to_reference(int32_t env_kind, uint32_t s) {
    if (env_kind == RL_ENV_BLACKJACK) return rl_blackjack_obs_id(s >> 6, (s >> 1) & 31u, s & 1u);
    return s;
}
int rl_obs_from_reference(int32_t env_kind, uint64_t obs, uint32_t *dense_state) {
    if (!dense_state) return fail(RL_E_ARG, "null argument");
    if (env_kind != RL_ENV_BLACKJACK) {
        if (obs > 0xffffffffull) return fail(RL_E_ARG, "observation out of range");
        *dense_state = (uint32_t)obs;
        return RL_OK;
    }
    // the 2048 dense Blackjack observations by their fxhash ids (distinct: checked once)
    static const std::vector<std::pair<uint64_t, uint32_t>> ids = [] {
        std::vector<std::pair<uint64_t, uint32_t>> v(2048);
        for (uint32_t s = 0; s < 2048; ++s) v[s] = {rl_obs_to_reference(RL_ENV_BLACKJACK, s), s};
        std::sort(v.begin(), v.end());
        return v;
    }();
    const auto it = std::lower_bound(ids.begin(), ids.end(), std::make_pair(obs, 0u));
    if (it == ids.end() || it->first != obs) return fail(RL_E_ARG, "not a Blackjack observation id");
    *dense_state = it->second;
    return RL_OK;
}

// rl_map_register / rl_map_register_wide: one validation and one registry; `cap` is
// the format's cell limit and `cap_name` its name in the messages
static int map_register(const char *const *rows, uint32_t n_rows, int32_t *map_id, size_t cap, const char *cap_name,
                        bool wide) {
    if (!rows || !map_id) return fail(RL_E_ARG, "null argument");
    if (n_rows == 0) return fail(RL_E_ARG, "a map needs at least one row");
    Grid g;
    for (uint32_t r = 0; r < n_rows; ++r) {
        if (!rows[r]) return fail(RL_E_ARG, "null map row " + std::to_string(r));
        // the length is bounded while it is measured: a row is never read past the cell limit
        const size_t len = strnlen(rows[r], cap + 1);
        if (len == 0) return fail(RL_E_ARG, "map row " + std::to_string(r) + " has zero columns");
        if (r > 0 && len != g[0].size())
            return fail(RL_E_ARG, "ragged map: row " + std::to_string(r) + " has " +
                                      (len > cap ? "more than " + std::to_string(cap) : std::to_string(len)) +
                                      " columns, row 0 has " + std::to_string(g[0].size()));
        if ((size_t)n_rows * len > cap)
            return fail(RL_E_ARG, std::string("map has more than ") + cap_name + " (" + std::to_string(cap) + ") cells");
        for (size_t i = 0; i < len; ++i) {
            const char ch = rows[r][i];
            if (ch != 'S' && ch != 'F' && ch != 'H' && ch != 'G')
                return fail(RL_E_ARG, std::string("map letter outside SFHG at row ") + std::to_string(r) + ", column " +
                                          std::to_string(i));
        }
        g.emplace_back(rows[r], len);
    }
    std::lock_guard<std::mutex> lock(g_map_mu);
    std::vector<Grid> &maps = map_registry();
    std::vector<uint8_t> &flags = map_wide_flags();
    for (size_t i = 2; i < maps.size(); ++i)
        if (maps[i] == g && (flags[i] != 0) == wide) { *map_id = (int32_t)i; return RL_OK; }
    if (maps.size() >= (size_t)INT32_MAX) return fail(RL_E_ARG, "map registry full");
    maps.push_back(std::move(g));
    flags.push_back(wide ? 1 : 0);
    *map_id = (int32_t)(maps.size() - 1);
    return RL_OK;
}

int rl_map_register(const char *const *rows, uint32_t n_rows, int32_t *map_id) {
    return map_register(rows, n_rows, map_id, RL_MAP_MAX_CELLS, "RL_MAP_MAX_CELLS", false);
}

int rl_map_register_wide(const char *const *rows, uint32_t n_rows, int32_t *map_id) {
    return map_register(rows, n_rows, map_id, RL_MAP_WIDE_MAX_CELLS, "RL_MAP_WIDE_MAX_CELLS", true);
}

int rl_map_is_wide(int32_t map_id, int32_t *wide) {
    if (!wide) return fail(RL_E_ARG, "null argument");
    Grid g;
    bool w = false;
    if (!map_lookup(map_id, g, &w))
        return fail(RL_E_ARG, "unknown FrozenLake map id " + std::to_string(map_id));
    *wide = w ? 1 : 0;
    return RL_OK;
}

int rl_map_info(int32_t map_id, uint32_t *n_rows, uint32_t *n_cols, char *cells, size_t n) {
    Grid g;
    if (!map_lookup(map_id, g))
        return fail(RL_E_ARG, "unknown FrozenLake map id " + std::to_string(map_id));
    const size_t nr = g.size(), nc = g[0].size();
    if (n_rows) *n_rows = (uint32_t)nr;
    if (n_cols) *n_cols = (uint32_t)nc;
    if (cells) {
        if (n != nr * nc) return fail(RL_E_ARG, "cells must hold rows * cols = " + std::to_string(nr * nc) + " chars");
        for (size_t r = 0; r < nr; ++r) std::memcpy(cells + r * nc, g[r].data(), nc);
    }
    return RL_OK;
}

int rl_env_dims(const rl_env_config *cfg, uint32_t *S, uint32_t *A) {
    if (!cfg || !S || !A) return fail(RL_E_ARG, "null argument");
    EnvHost e;
    int rc = build_env(*cfg, e);
    if (rc) return rc;
    *S = e.S;
    *A = e.A;
    return RL_OK;
}

int rl_env_table(const rl_env_config *cfg, double *prob, uint32_t *next, double *reward, uint8_t *term,
                 double *start) {
    if (!cfg) return fail(RL_E_ARG, "null config");
    EnvHost e;
    int rc = build_env(*cfg, e);
    if (rc) return rc;
    if (e.kind == RL_ENV_BLACKJACK) return fail(RL_E_ARG, "Blackjack has no transition table");
    for (uint32_t s = 0; s < e.S; ++s)
        for (uint32_t a = 0; a < e.A; ++a) {
            const uint32_t w = env_wide(e.kenv) ? 0u : e.trans[s * e.A + a];
            const size_t k = ((size_t)s * e.A + a) * 3;
            double pr[3] = {1.0, 0.0, 0.0};
            uint32_t nx[3] = {0, 0, 0};
            double rw[3] = {0.0, 0.0, 0.0};
            uint8_t tm[3] = {0, 0, 0};
            if (e.kind == RL_ENV_FROZEN_LAKE || e.kind == RL_ENV_FROZEN_LAKE_EDITED) {
                const bool edited = e.kind == RL_ENV_FROZEN_LAKE_EDITED;
                const char cell = e.map[s / e.ncol][s % e.ncol];
                if (env_wide(e.kenv)) {
                    // the wide words as the device steps them: direction (a + 3 + i) & 3 on
                    // a slippery map, a on a deterministic one; one outcome on 'G' / 'H'
                    const uint16_t *t16 = (const uint16_t *)e.trans.data();
                    const int n = (e.slippery && cell != 'G' && cell != 'H') ? 3 : 1;
                    for (int i = 0; i < n; ++i) {
                        const uint32_t o = t16[(size_t)s * 4 + (n == 3 ? ((a + 3u + (uint32_t)i) & 3u) : a)];
                        pr[i] = n == 3 ? 1.0 / 3.0 : 1.0;
                        nx[i] = o & WIDE_NEXT_MASK;
                        rw[i] = edited ? ((o & WIDE_REWARD) ? 10.0 : -1.0) : ((o & WIDE_REWARD) ? 1.0 : 0.0);
                        tm[i] = (o & WIDE_TERM) ? 1 : 0;
                    }
                } else {
                    const int n = (w >> 24) & 1 ? 3 : 1;
                    for (int i = 0; i < n; ++i) {
                        const uint32_t o = (w >> (8 * i)) & 0xffu;
                        pr[i] = n == 3 ? 1.0 / 3.0 : 1.0;
                        nx[i] = o & 63u;
                        rw[i] = edited ? ((o & 64u) ? 10.0 : -1.0) : ((o & 64u) ? 1.0 : 0.0);
                        tm[i] = (o & 128u) ? 1 : 0;
                    }
                }
                if (cell == 'G' || cell == 'H') rw[0] = 0.0;   // (1.0, s, 0.0, true) rows: never stepped from
            } else if (e.kind == RL_ENV_CLIFF_WALKING) {
                nx[0] = w & 63u;
                rw[0] = (w & 64u) ? -100.0 : -1.0;
                tm[0] = (w & 128u) ? 1 : 0;
            } else {
                nx[0] = w & 511u;
                const uint32_t rc2 = (w >> 9) & 3u;
                rw[0] = rc2 == 0 ? -1.0 : (rc2 == 1 ? -10.0 : 20.0);
                tm[0] = (w >> 11) & 1u;
            }
            for (int i = 0; i < 3; ++i) {
                if (prob) prob[k + i] = pr[i];
                if (next) next[k + i] = nx[i];
                if (reward) reward[k + i] = rw[i];
                if (term) term[k + i] = tm[i];
            }
        }
    if (start) std::memcpy(start, e.start.data(), e.S * sizeof(double));
    return RL_OK;
}

}  // extern "C"

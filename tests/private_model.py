"""An exact model of ONE private lane (group_size == 1) over one launch.

TEST INFRASTRUCTURE ONLY.  Shared mode is pinned by tests/step_model.py with
tests/select_model.py; this file is the same third statement for private mode:
the tabular and double-tabular policies, eligibility traces, Dyna-Q planning and
the NeuralPolicy.  It is written from DESIGN.md section 2 ("Private mode",
"NeuralPolicy", "FrozenLakeEditedEnv", the draw sites), include/rl.h and the
reference sources cited below; not from oracle/rlref.c and not from the kernels.
No oracle, library or ctypes call: Python ints and CPython floats in the
reference's operation order, no fused multiply-add, sums from 0.0 in index order.
The stream, the card rule, the five envs, argmax_first, ucb_scores and the IEEE
division / square root are select_model's and step_model's.

Inputs
------
Lane(...) takes the configuration, the seed and the GLOBAL lane id and carries
from creation what no getter exposes: the stream, the env, the pending (s, a),
whether a reset is due, the double flag, the trace rows in first-visit order and
the Dyna model.  Lane.launch(K, ...) takes the lane's state before the launch:
  q       P*S*A f64 bit patterns, [P][S][A] (tabular), or
  w       n_params floats [W1 n_in x H][b1 H][W2 H x A][b2 A] (neural)
  n, t    the lane's UCB counters N[S][A] and t
  eps     the lane's epsilon
For a network the feature table [S][n_in] (rl_net_features) and exp / tanh are
inputs of the constructor, ln(t) is one for UCB: fdlibm sequences the model cannot
form.  They are callables given by the caller, and every value used is kept in
Lane.used = {"exp": {x bits: value}, "tanh": ..., "ln": {t: value}} so that the
tests check each against a 50-digit value.  Sigmoid, swish and their derivatives
are composed here from exp.

Outputs
-------
Launch: records (K dicts with every rl_step_record field), q (bit patterns) or w,
n, t, eps after the launch, and the lane's share of rl_stats: train_steps,
train_episodes, reward_sum_q16.  compare(launch, recorded) reports the first
differing record as select_model.compare_records does: (step, field, predicted,
recorded).

What it restates
----------------
Schedule (src/agent.rs:83-101): a lane that needs a reset does env.reset() +
get_action: kind 1 (s, a; the rest 0).  Otherwise env.step(a) + get_action(s2) +
update: kind 2.  `term` (the env's own or the truncation) asks for a reset at
the next step.  A lane in a plain run() launch is never DONE.
Selection (one_step_agent.rs:48-51) on policy.predict of the lane's CURRENT values:
the double policy reads (alpha + beta) / 2 (double_tabular_policy.rs:31-39).
eps-greedy (uniform_epsilon_greed.rs:51-66): no draw at eps == 0, else the eps test
with its high word first, then the exploring draw or the first maximum.  UCB
(upper_confidence_bound.rs:29-42): the lane's own counters; n and t are
incremented at the selection, before the update reads them.
update (one_step_agent.rs:53-86, elegibility_traces_agent.rs:61-104):
td = (r + gamma * next) - V[s][a], V = get_values (the flagged table of the double
policy), next by SARSA, Q-learning or expected SARSA with the eps probabilities of
the epsilon BEFORE the decay or the UCB probabilities of the current counters.
Tabular: Q[s][a] += lr * x at once (tabular_policy.rs:36).  The double policy
writes the other table and flips the flag once per update.  Traces: E[s][a] += 1,
then every action of every visited state takes x = td * E in first-visit order and
E *= fl(gamma * lambda); the set empties on `term`.  Epsilon decays on `term` only.
Dyna (internal_model_agent.rs:46-79, random_model.rs:29-38): after the inner
update add_info keeps the FIRST (s2, r) of (s, a), in insertion order; then
planning_steps times: gen_range(0..len) by rand 0.8.5's sample_single_inclusive
(zone (n << lz(n)) - 1, reject while the low word of v * n exceeds it),
get_action(s2) of the drawn entry (its draws, or the argmax on the values as they
are NOW), update(.., terminated = false, ..).  A planning update flips the double
flag, increments the UCB counters, runs the trace sweep; none decays epsilon.
NeuralPolicy (neural_policy.rs:41-59, network.rs:61-80, layers.rs:90-105,
loss.rs:4-9, activation.rs:5-94): forward z_j = (0.0 + sum_k x_k W1[k][j]) + b1[j],
out_i = (0.0 + sum_j act1(z_j) W2[j][i]) + b2[i], y = act2(out); softmax is
exp(o - max) over an in-order sum and softmax_prime is softmax itself.
update(s, a, x): t = y; t[a] += x; fit: e2_i = act2'(out_i) * ((2 * (y_i - t_i)) / A),
input_error with the OLD W2, W2 -= lr * (0.0 + h e2), e1 = act1'(z) * ie,
W1 -= lr * (0.0 + x e1), b -= lr * e.  Every predict is recomputed from the
parameters: there is no cache here, so a kernel's cache has to be invisible.
Traces over a network make one fit per visited entry in first-visit order.

Outside the model
-----------------
The train() evaluate interleave (plain run() launches in RL_MODE_TRAIN only);
Agent::reset and the DenseLayer::new / reset weight draws (parameters are an
input); the per-call Agent surface; populations; exp, tanh, ln and the feature
table (checked inputs).

Mutations
---------
Lane(mutation=...) switches one rule to a plausible wrong one (negative controls):
  "last_kept"       add_info overwrites an entry instead of keeping the first
  "eps_first"       a planning step makes its eps test (and exploring draw) before
                    the index draw
  "plan_term"       a planning update passes the stored step's `terminated`
  "stale_argmax"    a planning argmax reads the values from before the previous
                    planning update
  "leaky_slope"     leaky_relu' has slope 0.1 below 0
  "w2_first"        W2 is updated before input_error reads it
  "trace_reverse"   the neural trace sweep runs last-visit first
  "forward_reused"  update's values of s are the forward get_action made of the same
                    state a step earlier, before the fit between them
"""
import select_model as selm
import step_model as sm

MUTATIONS = ("last_kept", "eps_first", "plan_term", "stale_argmax", "leaky_slope", "w2_first", "trace_reverse",
             "forward_reused")
ACTIVATIONS = ("linear", "tanh", "relu", "leaky_relu", "relu6", "leaky_relu6", "sigmoid", "softmax", "swish",
               "hard_swish")
# where act1' (or act1) changes its branch: the liveness conditions count both sides
KINKS = {"linear": (), "tanh": (0.0,), "relu": (0.0,), "leaky_relu": (0.0,), "relu6": (0.0, 6.0),
         "leaky_relu6": (0.0, 6.0), "sigmoid": (0.0,), "swish": (0.0,), "hard_swish": (-3.0, 0.0)}
PLAN_BATCH = 16
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- rand's gen_range
def gen_index_of(v, n):
    """(index, rejected) of one u64 v for gen_range(0..n): sample_single_inclusive"""
    zone = ((n << (64 - n.bit_length())) - 1) & M64
    m = v * n
    return m >> 64, (m & M64) > zone


# ---------------------------------------------------------------- activations
def _max(a, b):                     # f64::max as the reference's call sites use it
    return a if (a > b or b != b) else b


def _min(a, b):
    return a if (a < b or b != b) else b


class Net:
    """Network of the neural bin: Dense(n_in, H) -> act1 -> Dense(H, A) -> act2, mse"""

    def __init__(self, n_in, H, A, act1, act2, exp, tanh, used, mutation=None):
        if act1 not in ACTIVATIONS or act2 not in ACTIVATIONS or act1 == "softmax":
            raise ValueError((act1, act2))
        self.n_in, self.H, self.A, self.act1, self.act2 = n_in, H, A, act1, act2
        self._exp, self._tanh, self.used, self.mutation = exp, tanh, used, mutation
        self.n_params = n_in * H + H + H * A + A
        self.sides = {k: [0, 0] for k in KINKS[act1]}          # [z below or at the kink, z above]
        self.e1_nonzero = self.fits = 0

    def exp(self, x):
        v = float(self._exp(x))
        self.used["exp"][sm.f64_bits(x)] = v
        return v

    def tanh(self, x):
        v = float(self._tanh(x))
        self.used["tanh"][sm.f64_bits(x)] = v
        return v

    def sigmoid(self, v):
        return 1.0 / (1.0 + self.exp(-v))

    def f(self, act, v):
        if act == "tanh":
            return self.tanh(v)
        if act == "relu":
            return _max(v, 0.0)
        if act == "leaky_relu":
            return _max(v, 0.1 * v)
        if act == "relu6":
            return _min(_max(v, 0.0), 6.0)
        if act == "leaky_relu6":
            return _min(_max(v, 0.1 * v), 6.0)
        if act == "sigmoid":
            return self.sigmoid(v)
        if act == "swish":
            return v * self.sigmoid(v)
        if act == "hard_swish":
            return (v * _min(_max(v + 3.0, 0.0), 6.0)) / 6.0
        return v

    def fprime(self, act, v):
        if act == "tanh":
            t = self.tanh(v)
            return 1.0 - t * t
        if act == "relu":
            return 1.0 if v > 0.0 else 0.0
        if act == "leaky_relu":
            return 1.0 if v > 0.0 else (0.1 if self.mutation == "leaky_slope" else 0.01)
        if act == "relu6":
            return 1.0 if (v > 0.0 and v < 6.0) else 0.0
        if act == "leaky_relu6":
            return 1.0 if (v > 0.0 and v < 6.0) else 0.01
        if act == "sigmoid":
            s = self.sigmoid(v)
            return s * (1.0 - s)
        if act == "swish":
            e = self.exp(v)
            return sm.ieee_div(e * (v + e + 1.0), (e + 1.0) * (e + 1.0))
        if act == "hard_swish":
            return (2.0 * v + 3.0) / 6.0 if v > -3.0 else 0.0
        return 1.0

    def softmax(self, v):
        m = v[0]
        for x in v:
            if x > m:
                m = x
        e = [self.exp(x - m) for x in v]
        acc = 0.0
        for x in e:
            acc = acc + x
        return [sm.ieee_div(x, acc) for x in e]

    def layer(self, act, v):
        return self.softmax(v) if act == "softmax" else [self.f(act, x) for x in v]

    def layer_prime(self, act, v):
        return self.softmax(v) if act == "softmax" else [self.fprime(act, x) for x in v]

    def split(self, w):
        n_in, H, A = self.n_in, self.H, self.A
        o1, o2, o3 = n_in * H, n_in * H + H, n_in * H + H + H * A
        return 0, o1, o2, o3          # offsets of W1, b1, W2, b2

    def forward(self, w, x):
        """(z[H], h[H], out[A], y[A])"""
        n_in, H, A = self.n_in, self.H, self.A
        _, o1, o2, o3 = self.split(w)
        z = []
        for j in range(H):
            acc = 0.0
            for k in range(n_in):
                acc = acc + x[k] * w[k * H + j]
            z.append(acc + w[o1 + j])
        for v in z:
            for kink, side in self.sides.items():
                side[v > kink] += 1
        h = self.layer(self.act1, z)
        out = []
        for i in range(A):
            acc = 0.0
            for j in range(H):
                acc = acc + h[j] * w[o2 + j * A + i]
            out.append(acc + w[o3 + i])
        return z, h, out, self.layer(self.act2, out)

    def fit(self, w, x, target, lr):
        """Network::fit in place on the list w"""
        n_in, H, A = self.n_in, self.H, self.A
        _, o1, o2, o3 = self.split(w)
        z, h, out, y = self.forward(w, x)
        pr = self.layer_prime(self.act2, out)
        e2 = [pr[i] * ((2.0 * (y[i] - target[i])) / float(A)) for i in range(A)]

        def input_error():
            ie = []
            for j in range(H):
                acc = 0.0
                for i in range(A):
                    acc = acc + e2[i] * w[o2 + j * A + i]
                ie.append(acc)
            return ie

        ie = None if self.mutation == "w2_first" else input_error()
        for j in range(H):
            for i in range(A):
                w[o2 + j * A + i] = w[o2 + j * A + i] - lr * (0.0 + h[j] * e2[i])
        if ie is None:
            ie = input_error()
        for i in range(A):
            w[o3 + i] = w[o3 + i] - lr * e2[i]
        d1 = self.layer_prime(self.act1, z)
        e1 = [d1[j] * ie[j] for j in range(H)]
        for k in range(n_in):
            for j in range(H):
                w[k * H + j] = w[k * H + j] - lr * (0.0 + x[k] * e1[j])
        for j in range(H):
            w[o1 + j] = w[o1 + j] - lr * e1[j]
        self.fits += 1
        self.e1_nonzero += sum(1 for v in e1 if v != 0.0 and v == v)


# ---------------------------------------------------------------- the Dyna model
class RandomModel:
    """IndexMap<(s, a), (s2, r)>: insertion order, entry().or_insert"""

    def __init__(self, mutation=None):
        self.keys, self.values, self.mutation = [], {}, mutation
        self.kept_first = 0           # add_info met an entry with a DIFFERENT outcome and kept the first

    def add_info(self, s, a, r, s2, term=False):
        k = (s, a)
        if k in self.values:
            old = self.values[k]
            if old[0] != s2 or sm.f64_bits(old[1]) != sm.f64_bits(r):
                self.kept_first += 1
                if self.mutation == "last_kept":
                    self.values[k] = (s2, r, term)
            return
        self.keys.append(k)
        self.values[k] = (s2, r, term)

    def __len__(self):
        return len(self.keys)

    def at(self, i):
        s, a = self.keys[i]
        s2, r, term = self.values[(s, a)]
        return s, a, s2, r, term


class Launch:
    __slots__ = ("records", "q", "w", "n", "t", "eps", "train_steps", "train_episodes", "reward_sum_q16")


# ---------------------------------------------------------------- the lane
class Lane:
    def __init__(self, *, env, seed, lane, map8x8=0, slippery=0, max_steps=100, agent="one_step", policy="tabular",
                 selector="eps_greedy", algo="qlearning", lr=0.05, gamma=0.95, lam=0.5, ucb_c=0.5, eps_decay=0.0,
                 eps_final=0.0, decay_kind=0, plan_steps=0, net=None, ln=None, mutation=None):
        """net: None, or dict(n_in, hidden, act1, act2, features [S][n_in], exp, tanh);
        ln: t -> ln(float(t)) (UCB only)"""
        if mutation is not None and mutation not in MUTATIONS:
            raise ValueError(mutation)
        if agent not in ("one_step", "traces") or algo not in ("sarsa", "qlearning", "expected_sarsa"):
            raise ValueError((agent, algo))
        if policy not in ("tabular", "double", "neural") or (policy == "neural") != (net is not None):
            raise ValueError(policy)
        self.S, self.A, make = selm.make_env(env, map8x8, slippery, max_steps)
        self.rng = selm.Stream(seed, lane)
        self.env = make(self.rng)               # Blackjack's constructor draws from the lane's stream
        self.P = 2 if policy == "double" else 1
        self.traces, self.ucb, self.algo = agent == "traces", selector == "ucb", algo
        self.lr, self.gamma, self.lam, self.ucb_c = float(lr), float(gamma), float(lam), float(ucb_c)
        self.eps_decay, self.eps_final, self.decay_kind = float(eps_decay), float(eps_final), decay_kind
        self.plan_steps, self.mutation = int(plan_steps), mutation
        self.used = {"exp": {}, "tanh": {}, "ln": {}}
        self._ln = ln
        self.net = self.feat = None
        if net is not None:
            self.net = Net(net["n_in"], net["hidden"], self.A, net["act1"], net["act2"], net["exp"], net["tanh"],
                           self.used, mutation)
            self.feat = [[float(v) for v in row] for row in net["features"]]
            if len(self.feat) != self.S or any(len(r) != self.net.n_in for r in self.feat):
                raise ValueError("features must be [S][n_in]")
        # carried from creation
        self.need_reset, self.s, self.a, self.flag = True, 0, 0, True
        self.E = {}                             # state -> [E[s][0..A)], first-visit order
        self.model = RandomModel(mutation)
        self.epi_reward = 0.0
        self.q = self.w = self.n = None
        self.t, self.eps = 1, 0.0
        self._stale = None                      # "forward_reused": (state, y) of the latest get_action
        self._plan_view = None                  # "stale_argmax": the values before the previous planning update
        self.stats = dict.fromkeys(
            ("explore", "greedy", "eps_zero", "resets", "terminal", "truncated", "gen_rejects", "plan_explore",
             "plan_greedy", "plan_ucb", "plan_on_written_row", "plan_on_written_row_cross_batch", "same_state",
             "sweep_rows_max", "nonfinite_params"), 0)
        self.model_lens = set()                 # every length an index was drawn over

    # ---- values
    def ln_t(self):
        if self.t not in self.used["ln"]:
            self.used["ln"][self.t] = float(self._ln(self.t))
        return self.used["ln"][self.t]

    def row(self, tbl, s, view=None):
        """policy.get_values of one table"""
        if self.net is not None:
            return self.net.forward(self.w, self.feat[s])[3]
        q = self.q if view is None else view
        i0 = (tbl * self.S + s) * self.A
        return q[i0:i0 + self.A]

    def predict(self, s, view=None):
        if self.P == 2:
            return [(x + y) / 2.0 for x, y in zip(self.row(0, s, view), self.row(1, s, view))]
        return list(self.row(0, s, view))

    # ---- selection
    def select(self, s, planning=False, pre=None, view=None):
        """get_action(s).  pre: the "eps_first" mutation's (explore, action) drawn early"""
        st = self.stats
        if self.ucb:
            vals = self.predict(s, view)
            i0 = s * self.A
            a, _ = selm.argmax_first(selm.ucb_scores(vals, self.n[i0:i0 + self.A], self.ln_t(), self.ucb_c))
            self.n[i0 + a] += 1
            self.t += 1
            st["plan_ucb"] += planning
            self._stale = (s, vals)
            return a, True
        if pre is not None:
            explore, a = pre
        elif self.eps == 0.0:
            explore, a = False, None
            st["eps_zero"] += 1
        else:
            explore = self.rng.eps_test(self.eps)
            a = self.rng.uniform_usize(self.A) if explore else None
        if explore:
            st["plan_explore" if planning else "explore"] += 1
            return a, False
        st["plan_greedy" if planning else "greedy"] += 1
        vals = self.predict(s, view)
        self._stale = (s, vals)
        return selm.argmax_first(vals)[0], True

    def _draw_selection(self):
        if self.ucb:
            return None
        if self.eps == 0.0:
            return (False, None)
        explore = self.rng.eps_test(self.eps)
        return (explore, self.rng.uniform_usize(self.A) if explore else None)

    # ---- update
    def policy_update(self, tbl, s, a, x, written):
        if self.net is not None:
            xs = self.feat[s]
            y = list(self.net.forward(self.w, xs)[3])
            y[a] += x
            self.net.fit(self.w, xs, y, self.lr)
            return
        i = (tbl * self.S + s) * self.A + a
        new = self.q[i] + self.lr * x
        if written is not None and sm.f64_bits(new) != sm.f64_bits(self.q[i]):
            written.add(s)
        self.q[i] = new

    def update(self, s, a, r, term, s2, a2, written=None):
        A = self.A
        vt, ut = ((0, 1) if self.flag else (1, 0)) if self.P == 2 else (0, 0)
        row2 = list(self.row(vt, s2))
        if self.algo == "sarsa":
            nxt = row2[a2]
        elif self.algo == "qlearning":
            nxt = sm._first_max(row2)
        elif self.ucb:
            nxt = sm.expected_ucb(row2, self.n[s2 * A:s2 * A + A], self.ln_t(), self.ucb_c)
        else:
            nxt = sm.expected_eps_greedy(row2, self.eps)
        if (self.mutation == "forward_reused" and self.net is not None and self._stale_prev is not None
                and self._stale_prev[0] == s):
            cur = self._stale_prev[1]
        else:
            cur = self.row(vt, s)
        td = r + self.gamma * nxt - cur[a]
        if not self.traces:
            self.policy_update(ut, s, a, td, written)
        else:
            self.E.setdefault(s, [0.0] * A)[a] += 1.0
            gl = self.gamma * self.lam
            order = list(self.E.items())
            if self.mutation == "trace_reverse" and self.net is not None:
                order.reverse()
            self.stats["sweep_rows_max"] = max(self.stats["sweep_rows_max"], len(order))
            for o, ev in order:
                for b in range(A):
                    self.policy_update(ut, o, b, td * ev[b], written)
                    ev[b] *= gl
        if self.P == 2:
            self.flag = not self.flag
        if term:
            self.E = {}
            if not self.ucb:
                nw = self.eps * self.eps_decay if self.decay_kind == 1 else self.eps - self.eps_decay
                if not self.eps_final > nw:
                    self.eps = nw
        return td

    def plan(self):
        st = self.stats
        written = {}                         # state -> index of the first planning step that changed its row
        prev_view = None
        for i in range(self.plan_steps):
            n = len(self.model)
            pre = self._draw_selection() if self.mutation == "eps_first" else None
            while True:
                idx, rejected = gen_index_of(self.rng.u64(), n)
                if not rejected:
                    break
                st["gen_rejects"] += 1
            self.model_lens.add(n)
            ps, pa, ps2, pr, pterm = self.model.at(idx)
            view = prev_view if self.mutation == "stale_argmax" else None
            na, read = self.select(ps2, planning=True, pre=pre, view=view)
            if read and ps2 in written:
                st["plan_on_written_row"] += 1
                if written[ps2] // PLAN_BATCH < i // PLAN_BATCH:
                    st["plan_on_written_row_cross_batch"] += 1
            if self.mutation == "stale_argmax" and self.net is None:
                prev_view = list(self.q)
            now = set()
            self._stale_prev = None
            self.update(ps, pa, pr, pterm if self.mutation == "plan_term" else False, ps2, na, now)
            for o in now:
                written.setdefault(o, i)

    # ---- the launch
    def launch(self, K, *, q=None, w=None, n=None, t=1, eps=0.0):
        if (self.net is None) == (q is None) or (self.net is not None) == (w is None):
            raise ValueError("a tabular lane takes q, a neural lane w")
        if q is not None:
            if len(q) != self.P * self.S * self.A:
                raise ValueError("q must hold P*S*A bit patterns")
            self.q = [sm.f64_from_bits(int(u)) for u in q]
        else:
            if len(w) != self.net.n_params:
                raise ValueError("w must hold n_params values")
            self.w = [float(v) for v in w]
        self.n = [int(v) for v in n] if n is not None else [0] * (self.S * self.A)
        self.t, self.eps = int(t), float(eps)
        out = Launch()
        out.records, out.train_steps, out.train_episodes, out.reward_sum_q16 = [], 0, 0, 0
        st = self.stats
        for _ in range(K):
            if self.need_reset:
                self.s = self.env.reset(self.rng)
                self.a, _ = self.select(self.s)
                self.need_reset, self.epi_reward = False, 0.0
                st["resets"] += 1
                out.records.append(dict(kind=sm.KIND_RESET, mode=sm.MODE_TRAIN, s=self.s, a=self.a, s2=0, a2=0, r=0.0,
                                        term=0, td=0.0))
                continue
            before = self.env.n_trunc
            s2, r, term = self.env.step(self.a, self.rng)
            if self.env.n_trunc != before:
                st["truncated"] += 1
            elif term:
                st["terminal"] += 1
            self._stale_prev = self._stale
            a2, _ = self.select(s2)
            st["same_state"] += s2 == self.s
            td = self.update(self.s, self.a, r, term, s2, a2)
            if self.plan_steps:
                self.model.add_info(self.s, self.a, r, s2, bool(term))
                self.plan()
            out.records.append(dict(kind=sm.KIND_STEP, mode=sm.MODE_TRAIN, s=self.s, a=self.a, s2=s2, a2=a2, r=r,
                                    term=int(term), td=td))
            out.train_steps += 1
            self.epi_reward += r
            self.s, self.a = s2, a2
            if term:
                self.need_reset = True
                out.train_episodes += 1
                out.reward_sum_q16 += int(round(self.epi_reward * 65536.0))
        out.q = [sm.f64_bits(v) for v in self.q] if self.q is not None else None
        out.w = list(self.w) if self.w is not None else None
        if out.w is not None and any(v != v or v in (float("inf"), -float("inf")) for v in out.w):
            st["nonfinite_params"] += 1
        out.n, out.t, out.eps = list(self.n), self.t, self.eps
        return out

    _stale_prev = None


def compare(launch, recorded):
    """[(step, field, predicted, recorded)] of the FIRST differing record only"""
    if len(recorded) != len(launch.records):
        raise ValueError("recorded must hold one record per step")
    for k, (mine, got) in enumerate(zip(launch.records, recorded)):
        bad = [(k, f, mine[f], got[f]) for f in selm.FIELDS if not selm._same(f, mine[f], got[f])]
        if bad:
            return bad
    return []


def same_bits(a, b):
    """f64 bit patterns equal, any NaN equal to any NaN (private Q is not canonical)"""
    x, y = sm.f64_from_bits(a), sm.f64_from_bits(b)
    return a == b or (x != x and y != y)

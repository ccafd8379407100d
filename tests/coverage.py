"""Coverage conditions computed from rl_step_record arrays.

A parity case is only worth its GPU time while its records are live: TD errors
that are finite and non-zero, Q entries that move, entries that several lanes of
a learner group (and several groups) write in the same step or launch, resets
and terminal transitions inside the window.  measure() counts these from the
records of one run; the tests assert them on the ORACLE's records (need=, as in
tests/test_step_model.py), so a case that stops exercising its edge fails on
the CPU instead of passing quietly on the GPU.

The module shares its name with the PyPI `coverage` package, and tests/ is first on
sys.path (tests/conftest.py): under pytest-cov or coverage.py, `import coverage` in
tests/ would find whichever was imported first.  Neither is a dependency of this
suite; a run under them has to rename one side.
"""
import numpy as np

KIND_RESET, KIND_STEP, KIND_RESET_STEP = 1, 2, 3
MODE_TRAIN = 0


def measure(recs, G, q_default, q=None, sync_every=None):
    """recs: [n_steps, n_lanes] records of one run; G: the learner group size (lane
    // G is a lane's group; 1 = private agents); q: the table(s) after the run, any
    shape; sync_every: steps per launch (needed for changed_by_2_groups).

    Returns a dict:
      train_steps          training STEP records (kind >= 2, mode train)
      live_share           share of those whose td is finite and non-zero
      entries_changed      entries of q that differ from q_default (NaN counts)
      multi_contrib        (step, group, s, a) entries with >= 2 contributions
      max_contrib          the largest contribution count of one such entry
      changed_by_2_groups  (launch, s, a) entries that >= 2 groups moved (td != 0)
      max_abs_td           largest finite |td| of a training STEP record
      resets, terminals, kind3
                           RESET records, training STEP records with term set
                           (termination or truncation), kind-3 records
    """
    recs = np.asarray(recs)
    n_steps, L = recs.shape
    kind, td = recs["kind"], recs["td"]
    train = (kind >= KIND_STEP) & (recs["mode"] == MODE_TRAIN)
    n_train = int(train.sum())
    live = train & np.isfinite(td) & (td != 0.0)
    out = dict(train_steps=n_train, live_share=float(live.sum()) / n_train if n_train else 0.0)
    if q is not None:
        q = np.asarray(q, np.float64)
        out["entries_changed"] = int(np.count_nonzero(q.view(np.uint64) != np.float64(q_default).view(np.uint64)))
    step = np.broadcast_to(np.arange(n_steps, dtype=np.int64)[:, None], recs.shape)
    group = np.broadcast_to((np.arange(L, dtype=np.int64) // G)[None, :], recs.shape)
    s, a = recs["s"].astype(np.int64), recs["a"].astype(np.int64)
    keys = np.stack([step[train], group[train], s[train], a[train]], axis=1)
    counts = np.unique(keys, axis=0, return_counts=True)[1] if n_train else np.zeros(0, np.int64)
    out["multi_contrib"] = int((counts >= 2).sum())
    out["max_contrib"] = int(counts.max(initial=0))
    if sync_every:
        moved = train & (td != 0.0)                    # NaN moves an entry too
        k4 = np.unique(np.stack([step[moved] // sync_every, s[moved], a[moved], group[moved]], axis=1), axis=0)
        per_entry = np.unique(k4[:, :3], axis=0, return_counts=True)[1] if len(k4) else np.zeros(0, np.int64)
        out["changed_by_2_groups"] = int((per_entry >= 2).sum())
    fin = td[train & np.isfinite(td)]
    out["max_abs_td"] = float(np.abs(fin).max(initial=0.0))
    out["resets"] = int((kind == KIND_RESET).sum())
    out["terminals"] = int((train & (recs["term"] != 0)).sum())
    out["kind3"] = int((kind == KIND_RESET_STEP).sum())
    return out


def assert_live(m, *, live_share=0.9, entries_changed=6, multi_contrib=50, resets=0, terminals=0,
                max_contrib=0, kind3=0):
    """the shared-mode conditions of the parity matrix; every bound is a minimum"""
    need = dict(live_share=live_share, entries_changed=entries_changed, multi_contrib=multi_contrib,
                resets=resets, terminals=terminals, max_contrib=max_contrib, kind3=kind3)
    short = {k: (m.get(k), v) for k, v in need.items() if v and not m.get(k, 0) >= v}
    assert not short, f"the case no longer exercises (measured, needed): {short}"

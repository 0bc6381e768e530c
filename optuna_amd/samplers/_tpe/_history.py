"""Incremental trial-history mirror for TPE (K10 "reduce/split" support).

The reference rebuilds per-suggest Python lists over the whole history
(reference ``optuna/samplers/_tpe/sampler.py`` :564-574 `_get_internal_repr`);
at a 10k-trial history that loop dominates suggest latency. Here each sampler
keeps an append-only SoA mirror of finished trials:

* master table: number, state, objective values, constraint-violation sum,
  pruned-trial score — appended once when a trial is first seen finished;
* per-search-space parameter matrices (internal repr) with validity masks,
  appended in lockstep.

The below/above split then becomes a handful of numpy argsorts over resident
arrays, and the observation matrices for the Parzen fit are row gathers. On a
GPU box the same arrays are mirrored into device memory by ``optuna_amd._hip``
(uploaded incrementally, resident in HBM) so the K1/K2 kernels read them with no
per-suggest host→device traffic of the full history.

Finished trials are immutable (storage contract, storages/_base.py), which is
what makes the append-only mirror sound.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Sequence

import numpy as np

from optuna_amd.distributions import BaseDistribution
from optuna_amd.study._study_direction import StudyDirection
from optuna_amd.trial import FrozenTrial, TrialState


if TYPE_CHECKING:
    from optuna_amd.study import Study

_CHUNK = 4096  # growth granularity of the SoA arrays


class _SpaceCache:
    """Per-search-space internal-repr matrix aligned with the master table rows.

    Alongside the raw matrix it maintains, per dimension, the list of valid row
    indices sorted by parameter value (kept sorted incrementally). The Parzen fit
    needs neighbor gaps in sorted order; supplying these orders removes the
    per-suggest O(N log N) argsort per dimension.
    """

    def __init__(self, space: dict[str, BaseDistribution]) -> None:
        self.space = dict(space)
        self.names = list(space.keys())
        self.dists = [space[n] for n in self.names]
        # Capacity-doubled row store: `params`/`valid` are views of the filled
        # prefix, so a per-tell append is a row write, not an O(N) reallocation.
        self._n_rows = 0
        self._params_buf = np.empty((64, len(self.names)), dtype=np.float64)
        self._valid_buf = np.empty(64, dtype=bool)
        # Per-dim sorted index kept in capacity-doubled buffers: the per-tell
        # insert is a searchsorted + tail shift, avoiding np.insert's full
        # reallocation per dimension per suggest.
        # Rows as int32: the device compaction kernels consume these columns
        # directly (contiguous per-dim prefixes, no per-suggest restack/cast).
        # The host index is maintained lazily: `append` only records the new
        # valid rows, and the accessors below (`sorted_vals`, `sorted_rows`,
        # `_n_sorted`) replay the backlog first. A suggest that runs on the
        # device-resident index never pays the per-dim tail shifts.
        self._n_sorted_host = 0
        self._vals_buf = [np.empty(64, dtype=np.float64) for _ in self.names]
        self._rows_buf = [np.empty(64, dtype=np.int32) for _ in self.names]
        self._pending: list[np.ndarray] = []  # valid rows per append, unflushed
        # Non-flushing counters: valid rows so far, and the invalid row ids
        # (rows whose trial lacks a parameter of the space), ascending.
        self.n_valid = 0
        self._invalid_rows: list[int] = []
        self._invalid_arr = np.empty(0, dtype=np.int32)

    @property
    def params(self) -> np.ndarray:
        return self._params_buf[: self._n_rows]

    @property
    def valid(self) -> np.ndarray:
        return self._valid_buf[: self._n_rows]

    @property
    def sorted_vals(self) -> list[np.ndarray]:
        self._flush()
        return [b[: self._n_sorted_host] for b in self._vals_buf]

    @property
    def sorted_rows(self) -> list[np.ndarray]:
        self._flush()
        return [b[: self._n_sorted_host] for b in self._rows_buf]

    @property
    def _n_sorted(self) -> int:
        self._flush()
        return self._n_sorted_host

    @property
    def n_invalid(self) -> int:
        return len(self._invalid_rows)

    def excluded_rows(self, below_rows: np.ndarray) -> np.ndarray:
        """Sorted int32 table rows outside the "above" set when that set is the
        ascending-row complement of ``below_rows``: the below rows plus the
        rows invalid for this space. O(n_below + n_invalid)."""
        excl = np.sort(np.asarray(below_rows)).astype(np.int32)
        if self._invalid_rows:
            if len(self._invalid_arr) != len(self._invalid_rows):
                self._invalid_arr = np.asarray(self._invalid_rows, dtype=np.int32)
            excl = np.union1d(excl, self._invalid_arr)
        return excl

    def append(self, trials: Sequence[FrozenTrial]) -> None:
        n_new = len(trials)
        if n_new == 0:
            return
        base = self._n_rows
        if base + n_new > len(self._valid_buf):
            cap = max(2 * len(self._valid_buf), base + n_new)
            pb = np.empty((cap, len(self.names)), dtype=np.float64)
            vb_ = np.empty(cap, dtype=bool)
            pb[:base] = self._params_buf[:base]
            vb_[:base] = self._valid_buf[:base]
            self._params_buf = pb
            self._valid_buf = vb_
        block = self._params_buf[base : base + n_new]
        valid = self._valid_buf[base : base + n_new]
        for r, t in enumerate(trials):
            params = t.params
            ok = True
            for c, (name, dist) in enumerate(zip(self.names, self.dists)):
                if name in params:
                    block[r, c] = dist.to_internal_repr(params[name])
                else:
                    ok = False
                    break
            valid[r] = ok
        self._n_rows = base + n_new

        new_rows = base + np.nonzero(valid)[0]
        m = len(new_rows)
        if m < n_new:
            self._invalid_rows.extend((base + np.nonzero(~valid)[0]).tolist())
        if m == 0:
            return
        self.n_valid += m
        self._pending.append(new_rows)

    def _flush(self) -> None:
        """Bring the host sorted index up to date, one recorded append at a
        time (so the arrays equal eager maintenance)."""
        if self._pending:
            pending, self._pending = self._pending, []
            for new_rows in pending:
                self._insert_sorted(new_rows)

    def _insert_sorted(self, new_rows: np.ndarray) -> None:
        m = len(new_rows)
        n = self._n_sorted_host
        if n + m > len(self._vals_buf[0]):
            cap = max(2 * len(self._vals_buf[0]), n + m)
            for c in range(len(self.names)):
                vb = np.empty(cap, dtype=np.float64)
                rb = np.empty(cap, dtype=np.int32)
                vb[:n] = self._vals_buf[c][:n]
                rb[:n] = self._rows_buf[c][:n]
                self._vals_buf[c] = vb
                self._rows_buf[c] = rb
        for c in range(len(self.names)):
            vb = self._vals_buf[c]
            rb = self._rows_buf[c]
            vals = self.params[new_rows, c]
            if m == 1:
                # side="right": equal values keep insertion (= row) order.
                # The tail shift moves right, which numpy handles in place for
                # fp64/int32 strided slices only via an explicit reversed copy;
                # one reusable scratch avoids two 80 KB allocations per tell.
                i = int(np.searchsorted(vb[:n], vals[0], side="right"))
                tail = n - i
                sf, si = self._shift_scratch or (None, None)
                if sf is None or len(sf) < tail:
                    sf = np.empty(max(1024, 2 * tail), dtype=np.float64)
                    si = np.empty(max(1024, 2 * tail), dtype=np.int32)
                    self._shift_scratch = (sf, si)
                sf[:tail] = vb[i:n]
                vb[i + 1 : n + 1] = sf[:tail]
                si[:tail] = rb[i:n]
                rb[i + 1 : n + 1] = si[:tail]
                vb[i] = vals[0]
                rb[i] = new_rows[0]
            else:
                order = np.argsort(vals, kind="stable")
                vals_sorted = vals[order]
                rows_sorted = new_rows[order]
                pos = np.searchsorted(vb[:n], vals_sorted, side="right")
                merged_v = np.insert(vb[:n], pos, vals_sorted)
                merged_r = np.insert(rb[:n], pos, rows_sorted)
                vb[: n + m] = merged_v
                rb[: n + m] = merged_r
        self._n_sorted_host = n + m

    _shift_scratch: tuple[np.ndarray, np.ndarray] | None = None


class _TpeHistory:
    """Append-only mirror of one study's finished trials (see module docstring)."""

    def __init__(self) -> None:
        # Master SoA columns live in capacity-doubled buffers; the public
        # `_numbers` etc. are views of the filled prefix (appends are row
        # writes, not O(N) reallocations per tell).
        self._m_n = 0
        self._m_cap = 64
        self._numbers_buf = np.empty(64, dtype=np.int64)
        self._states_buf = np.empty(64, dtype=np.int8)
        self._values_buf: np.ndarray | None = None  # (cap, M)
        self._violations_buf = np.empty(64, dtype=np.float64)
        self._pruned_step_buf = np.empty(64, dtype=np.float64)
        self._pruned_value_buf = np.empty(64, dtype=np.float64)
        self._has_intermediate_buf = np.empty(64, dtype=bool)
        self._seen: set[int] = set()
        self._trials: list[FrozenTrial] = []  # row-aligned frozen trials
        self._spaces: dict[tuple, _SpaceCache] = {}
        # Rows appended in trial-number order? (True until proven otherwise; lets
        # split() order the big "above" set with a boolean mask instead of argsort.)
        self._rows_number_ascending = True
        # Incrementally-sorted feasible-complete rows by objective value (single-
        # objective minimize fast path for split(); ties keep row order, matching
        # a stable argsort).
        self._comp_vals = np.empty(0, dtype=np.float64)
        self._comp_rows = np.empty(0, dtype=np.int64)
        self._comp_cache_valid = True
        # Split memo: independent-mode TPE (e.g. multi-objective) runs one
        # _sample per dimension within a single suggest; the history is
        # unchanged between them, so the (rows, gamma) split — including the
        # K6 non-domination rank — is identical and cached per (n, n_below).
        self._split_memo: tuple[int, int, np.ndarray, np.ndarray] | None = None

    def __len__(self) -> int:
        return self._m_n

    @property
    def _numbers(self) -> np.ndarray:
        return self._numbers_buf[: self._m_n]

    @property
    def _states(self) -> np.ndarray:
        return self._states_buf[: self._m_n]

    @property
    def _values(self) -> np.ndarray | None:
        return None if self._values_buf is None else self._values_buf[: self._m_n]

    @property
    def _violations(self) -> np.ndarray:
        return self._violations_buf[: self._m_n]

    @property
    def _pruned_step(self) -> np.ndarray:
        return self._pruned_step_buf[: self._m_n]

    @property
    def _pruned_value(self) -> np.ndarray:
        return self._pruned_value_buf[: self._m_n]

    @property
    def _has_intermediate(self) -> np.ndarray:
        return self._has_intermediate_buf[: self._m_n]

    @property
    def trials(self) -> list[FrozenTrial]:
        return self._trials

    def update(
        self, finished: Sequence[FrozenTrial], n_objectives: int, delta: bool = False
    ) -> None:
        """Append trials not yet mirrored.

        With ``delta=True``, ``finished`` is a partial list (e.g. from
        ``InMemoryStorage.get_finished_trials_since``) and is deduped directly.
        Otherwise it is the complete finished list: the scan runs backwards and
        stops once the known number of new trials is found — new trials usually
        sit at the tail, so the common case touches O(new) entries, not
        O(history).
        """
        if delta:
            new = [t for t in finished if t._trial_id not in self._seen]
        else:
            n_missing = len(finished) - len(self._seen)
            if n_missing <= 0:
                return  # seen ⊆ finished and same cardinality ⇒ nothing new
            if n_missing == len(finished):
                new = list(finished)
            else:
                new = []
                for t in reversed(finished):
                    if t._trial_id not in self._seen:
                        new.append(t)
                        if len(new) == n_missing:
                            break
                new.reverse()
        if not new:
            return
        n_new = len(new)
        numbers = np.fromiter((t.number for t in new), dtype=np.int64, count=n_new)
        states = np.fromiter((int(t.state) for t in new), dtype=np.int8, count=n_new)
        values = np.full((n_new, n_objectives), np.nan, dtype=np.float64)
        violations = np.zeros(n_new, dtype=np.float64)
        p_step = np.full(n_new, np.nan)
        p_value = np.full(n_new, np.nan)
        has_iv = np.zeros(n_new, dtype=bool)
        for r, t in enumerate(new):
            if t.values is not None and len(t.values) == n_objectives:
                values[r] = t.values
            constraints = t.system_attrs.get("constraints")
            if constraints is not None:
                violations[r] = sum(v for v in constraints if v > 0)
            if t.intermediate_values:
                step, iv = max(t.intermediate_values.items())
                p_step[r] = step
                p_value[r] = iv
                has_iv[r] = True
            self._seen.add(t._trial_id)

        if self._rows_number_ascending:
            prev_last = self._numbers_buf[self._m_n - 1] if self._m_n else -1
            if numbers[0] <= prev_last or (n_new > 1 and np.any(np.diff(numbers) <= 0)):
                self._rows_number_ascending = False

        base_m = self._m_n
        if self._values_buf is None:
            self._values_buf = np.empty((self._m_cap, n_objectives), dtype=np.float64)
        if base_m + n_new > self._m_cap:
            cap = max(2 * self._m_cap, base_m + n_new)
            for attr in (
                "_numbers_buf",
                "_states_buf",
                "_violations_buf",
                "_pruned_step_buf",
                "_pruned_value_buf",
                "_has_intermediate_buf",
                "_values_buf",
            ):
                old = getattr(self, attr)
                grown = np.empty((cap,) + old.shape[1:], dtype=old.dtype)
                grown[:base_m] = old[:base_m]
                setattr(self, attr, grown)
            self._m_cap = cap
        self._numbers_buf[base_m : base_m + n_new] = numbers
        self._states_buf[base_m : base_m + n_new] = states
        self._values_buf[base_m : base_m + n_new] = values
        self._violations_buf[base_m : base_m + n_new] = violations
        self._pruned_step_buf[base_m : base_m + n_new] = p_step
        self._pruned_value_buf[base_m : base_m + n_new] = p_value
        self._has_intermediate_buf[base_m : base_m + n_new] = has_iv
        self._m_n = base_m + n_new
        self._trials.extend(new)
        for cache in self._spaces.values():
            cache.append(new)

        if self._comp_cache_valid:
            if n_objectives != 1:
                self._comp_cache_valid = False
            else:
                base = self._m_n - n_new
                fc = np.nonzero(
                    (states == int(TrialState.COMPLETE)) & (violations <= 0)
                )[0]
                if fc.size:
                    vals = values[fc, 0]
                    if np.any(np.isnan(vals)):
                        self._comp_cache_valid = False
                    else:
                        order = np.argsort(vals, kind="stable")
                        vs = vals[order]
                        rs = (base + fc)[order]
                        # side="right": equal values keep insertion (= row) order,
                        # matching a stable argsort over the full column.
                        pos = np.searchsorted(self._comp_vals, vs, side="right")
                        self._comp_vals = np.insert(self._comp_vals, pos, vs)
                        self._comp_rows = np.insert(self._comp_rows, pos, rs)

    # ---- split ---------------------------------------------------------------------

    def split(self, study: "Study", n_below: int) -> tuple[np.ndarray, np.ndarray]:
        """Vectorized `_split_trials` over the mirror; returns (below_rows, above_rows).

        Exactly mirrors reference sampler.py:740-882: feasible completes ranked by
        value (MO: non-domination rank + HSSP tie-break), then pruned trials by
        (-last_step, signed value), then infeasible by violation; stable order.
        """
        directions = study.directions
        n = len(self._numbers)
        n_below_arg = n_below  # n_below is consumed section-by-section below
        memo = self._split_memo
        if memo is not None and memo[0] == n and memo[1] == n_below_arg:
            return memo[2], memo[3]
        rows = np.arange(n)
        is_infeasible = self._violations > 0
        is_complete = (self._states == int(TrialState.COMPLETE)) & ~is_infeasible
        is_pruned = (self._states == int(TrialState.PRUNED)) & ~is_infeasible

        below_parts: list[np.ndarray] = []
        above_parts: list[np.ndarray] = []

        # 1. complete trials
        if (
            len(directions) == 1
            and directions[0] != StudyDirection.MAXIMIZE
            and self._comp_cache_valid
        ):
            # Minimize fast path: feasible completes are kept value-sorted
            # incrementally, so the O(N log N) argsort per suggest disappears.
            comp_rows = self._comp_rows
            k = min(n_below, len(comp_rows))
            below_parts.append(comp_rows[:k])
            above_parts.append(comp_rows[k:])
        elif len(directions) <= 1:
            comp_rows = rows[is_complete]
            k = min(n_below, len(comp_rows))
            assert self._values is not None
            vals = self._values[comp_rows, 0]
            sign = -1.0 if directions[0] == StudyDirection.MAXIMIZE else 1.0
            order = np.argsort(sign * vals, kind="stable")
            below_parts.append(comp_rows[order[:k]])
            above_parts.append(comp_rows[order[k:]])
        else:
            comp_rows = rows[is_complete]
            k = min(n_below, len(comp_rows))
            below_c, above_c = self._split_complete_mo(comp_rows, directions, k)
            below_parts.append(below_c)
            above_parts.append(above_c)
        n_below = max(0, n_below - k)

        # 2. pruned trials: score = (-last_step, signed value); no intermediates → (1, 0)
        pr = rows[is_pruned]
        if len(pr):
            sign = (
                -1.0
                if len(directions) == 1 and directions[0] == StudyDirection.MAXIMIZE
                else 1.0
            )
            primary = np.where(self._has_intermediate[pr], -self._pruned_step[pr], 1.0)
            sv = sign * self._pruned_value[pr]
            secondary = np.where(
                self._has_intermediate[pr], np.where(np.isnan(sv), np.inf, sv), 0.0
            )
            order = np.lexsort((secondary, primary))
            k = min(n_below, len(pr))
            below_parts.append(pr[order[:k]])
            above_parts.append(pr[order[k:]])
            n_below = max(0, n_below - k)

        # 3. infeasible trials by violation
        inf_rows = rows[is_infeasible]
        if len(inf_rows):
            order = np.argsort(self._violations[inf_rows], kind="stable")
            k = min(n_below, len(inf_rows))
            below_parts.append(inf_rows[order[:k]])
            above_parts.append(inf_rows[order[k:]])

        below = np.concatenate(below_parts) if below_parts else np.empty(0, dtype=np.int64)
        # Estimator observations are ordered by trial number. `below` is small
        # (the gamma quantile); `above` is everything else, so when rows were
        # appended number-ascending its number order is just the row-order
        # complement of `below` — a boolean mask instead of an O(N log N) sort.
        below = below[np.argsort(self._numbers[below], kind="stable")]
        if self._rows_number_ascending:
            mask = np.ones(n, dtype=bool)
            mask[below] = False
            above = rows[mask]
        else:
            above = (
                np.concatenate(above_parts) if above_parts else np.empty(0, dtype=np.int64)
            )
            above = above[np.argsort(self._numbers[above], kind="stable")]
        self._split_memo = (n, n_below_arg, below, above)
        return below, above

    def _split_complete_mo(
        self, comp_rows: np.ndarray, directions: Sequence[StudyDirection], n_below: int
    ) -> tuple[np.ndarray, np.ndarray]:
        from optuna_amd._hypervolume.hssp import _solve_hssp
        from optuna_amd.samplers._tpe.sampler import _get_reference_point
        from optuna_amd.study._multi_objective import _fast_non_domination_rank

        if n_below == 0:
            return np.empty(0, dtype=np.int64), comp_rows
        if n_below >= len(comp_rows):
            return comp_rows, np.empty(0, dtype=np.int64)
        assert self._values is not None
        lvals = self._values[comp_rows].copy()
        lvals *= np.array(
            [-1.0 if d == StudyDirection.MAXIMIZE else 1.0 for d in directions]
        )
        ranks = _fast_non_domination_rank(lvals, n_below=n_below)
        uniq, counts = np.unique(ranks, return_counts=True)
        last_full = int(np.max(uniq[np.cumsum(counts) <= n_below], initial=-1))
        local = np.arange(len(comp_rows))
        sel = local[ranks <= last_full]
        if sel.size < n_below:
            need = ranks == last_full + 1
            cand_lvals = lvals[need]
            subset = n_below - sel.size
            chosen = _solve_hssp(
                cand_lvals, local[need], subset, _get_reference_point(cand_lvals)
            )
            sel = np.append(sel, chosen)
        mask = np.zeros(len(comp_rows), dtype=bool)
        mask[sel] = True
        return comp_rows[mask], comp_rows[~mask]

    # ---- observations ---------------------------------------------------------------

    def space_cache(self, space: dict[str, BaseDistribution]) -> _SpaceCache:
        key = tuple((n, d) for n, d in space.items())
        cache = self._spaces.get(key)
        if cache is None:
            cache = _SpaceCache(space)
            cache.append(self._trials)
            self._spaces[key] = cache
        return cache

    def valid_rows(
        self,
        space: dict[str, BaseDistribution],
        row_indices: np.ndarray,
        cache: _SpaceCache | None = None,
    ) -> np.ndarray:
        """Subset of row_indices whose trials define every parameter of the space."""
        if cache is None:
            cache = self.space_cache(space)
        return row_indices[cache.valid[row_indices]]

    def observations(
        self,
        space: dict[str, BaseDistribution],
        row_indices: np.ndarray,
        cache: _SpaceCache | None = None,
    ) -> tuple[dict[str, np.ndarray], dict[str, np.ndarray]]:
        """Row-gather the observation matrix for a trial subset.

        Returns (observations, sorted_orders): per-param value arrays in trial-number
        order, plus per-param argsort arrays derived from the incrementally-sorted
        index (no per-call sort).
        """
        if cache is None:
            cache = self.space_cache(space)
        sel = row_indices[cache.valid[row_indices]]
        mat = cache.params[sel]
        obs = {name: mat[:, c] for c, name in enumerate(cache.names)}

        n_total = len(cache.valid)
        if len(sel) * 16 < n_total:
            # Tiny subset (e.g. the "below" gamma quantile): sorting it directly
            # is cheaper than filtering the full presorted index per dimension.
            orders_small = {
                name: np.argsort(mat[:, c], kind="stable")
                for c, name in enumerate(cache.names)
            }
            return obs, orders_small
        in_sel = np.zeros(n_total, dtype=bool)
        in_sel[sel] = True
        pos = np.empty(n_total, dtype=np.int64)
        pos[sel] = np.arange(len(sel))
        orders = {}
        for c, name in enumerate(cache.names):
            sr = cache.sorted_rows[c]
            orders[name] = pos[sr[in_sel[sr]]]
        return obs, orders

"""Distributed trial-table storage: conformance + multi-process (gloo-style) tests."""
from __future__ import annotations

import datetime
import multiprocessing
import socket

import pytest

import optuna_amd
from optuna_amd.storages import BaseStorage
from optuna_amd.testing.pytest_storages import StorageTestCase


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _make_store(port: int, world_size: int, is_master: bool):
    import time

    from torch.distributed import TCPStore

    # The free-port probe races other tests/processes; the master retries a
    # failed bind a few times before giving up.
    last: Exception | None = None
    for _ in range(5):
        try:
            return TCPStore(
                "127.0.0.1",
                port,
                world_size,
                is_master=is_master,
                timeout=datetime.timedelta(seconds=60),
            )
        except (RuntimeError, OSError) as e:
            last = e
            if not is_master:
                raise
            time.sleep(0.5)
    raise RuntimeError(f"TCPStore bind failed on {port}: {last}")


class TestRcclStorageConformance(StorageTestCase):
    @pytest.fixture
    def storage(self) -> BaseStorage:
        from optuna_amd.storages._rccl import RcclStorage

        store = _make_store(_free_port(), 1, True)
        s = RcclStorage(store)
        s._store = store
        return s


def _worker(rank: int, world_size: int, port: int, queue) -> None:
    try:
        import warnings

        warnings.simplefilter("ignore")
        from optuna_amd.storages._rccl import RcclStorage

        optuna_amd.logging.set_verbosity(optuna_amd.logging.WARNING)
        store = _make_store(port, world_size, rank == 0)
        storage = RcclStorage(store, worker_label=f"rank{rank}")
        if rank == 0:
            study = optuna_amd.create_study(
                study_name="dist", storage=storage,
                sampler=optuna_amd.samplers.TPESampler(seed=rank, n_startup_trials=3),
            )
            store.set("study_ready", "1")
        else:
            store.get("study_ready")  # blocks until created
            study = optuna_amd.load_study(
                study_name="dist", storage=storage,
                sampler=optuna_amd.samplers.TPESampler(seed=rank, n_startup_trials=3),
            )

        def objective(trial):
            x = trial.suggest_float("x", -5, 5)
            y = trial.suggest_float("y", -5, 5)
            return x * x + y * y

        study.optimize(objective, n_trials=8)
        # Barrier: wait until every worker finished its 8 trials before counting.
        store.add("done", 1)
        import time

        while store.add("done", 0) < world_size:
            time.sleep(0.01)
        # Reads are rate-limited and may serve a view up to 25 sync TTLs old;
        # the other worker's last tell can be younger than that, so pull the
        # log's tail before counting.
        storage._sync(force=True)
        trials = study.get_trials(deepcopy=False)
        queue.put((rank, len(trials), [t.number for t in trials]))
        # The rank-0 process hosts the TCPStore: keep it alive until every
        # worker is done with store operations.
        store.add("exit", 1)
        if rank == 0:
            while store.add("exit", 0) < world_size:
                time.sleep(0.01)
    except Exception as e:  # surface the failure to the parent
        import traceback

        queue.put((rank, -1, traceback.format_exc()))


def test_two_process_shared_study() -> None:
    """world_size=2: both workers optimize one study; numbering stays dense."""
    port = _free_port()
    ctx = multiprocessing.get_context("spawn")
    queue = ctx.Manager().Queue()
    procs = [
        ctx.Process(target=_worker, args=(rank, 2, port, queue)) for rank in range(2)
    ]
    for p in procs:
        p.daemon = True
        p.start()
    for p in procs:
        p.join(timeout=180)
    for p in procs:
        if p.is_alive():
            p.terminate()
    results = [queue.get(timeout=10) for _ in range(2)]
    for rank, n, payload in results:
        assert n != -1, f"rank {rank} failed:\n{payload}"
        assert n == 16  # both workers see all 16 trials
        assert payload == list(range(16))  # dense, consecutive numbering


def _claim_worker(rank: int, world_size: int, port: int, trial_id: int, queue) -> None:
    try:
        from optuna_amd.storages._rccl import RcclStorage
        from optuna_amd.trial import TrialState

        store = _make_store(port, world_size, rank == 0)
        storage = RcclStorage(store, worker_label=f"claim{rank}")
        if rank == 0:
            study_id = storage.create_new_study(
                [optuna_amd.study.StudyDirection.MINIMIZE], study_name="cas"
            )
            tid = storage.create_new_trial(
                study_id, template_trial=optuna_amd.create_trial(state=TrialState.WAITING)
            )
            store.set("trial_id", str(tid))
        tid = int(store.get("trial_id"))
        store.add("barrier", 1)
        import time as _time

        deadline = _time.monotonic() + 60
        while store.add("barrier", 0) < world_size:
            _time.sleep(0.005)
            if _time.monotonic() > deadline:
                raise TimeoutError("barrier timeout")
        won = storage.set_trial_state_values(tid, TrialState.RUNNING)
        queue.put((rank, bool(won)))
        store.add("exit", 1)
        if rank == 0:
            import time

            while store.add("exit", 0) < world_size:
                time.sleep(0.01)
    except Exception:
        import traceback

        queue.put((rank, traceback.format_exc()))


def test_waiting_claim_cas_across_processes() -> None:
    """Exactly one of N processes wins the WAITING→RUNNING claim."""
    ctx = multiprocessing.get_context("spawn")
    world = 3
    last_error = ""
    # Under a loaded full-suite run the freshly probed port can be stolen by
    # another test before the master binds it; retry the whole round on a new
    # port instead of failing on infrastructure.
    for _attempt in range(3):
        port = _free_port()
        queue = ctx.Manager().Queue()
        procs = [
            ctx.Process(target=_claim_worker, args=(rank, world, port, 0, queue))
            for rank in range(world)
        ]
        for p in procs:
            p.daemon = True
            p.start()
        for p in procs:
            p.join(timeout=120)
        for p in procs:
            if p.is_alive():
                p.terminate()
        results = []
        while len(results) < world:
            try:
                results.append(queue.get(timeout=10))
            except Exception:
                break
        wins = [won for _rank, won in results if isinstance(won, bool)]
        if len(wins) == world:
            assert sum(wins) == 1
            return
        last_error = "\n".join(str(w) for _r, w in results if not isinstance(w, bool))
    pytest.fail(f"CAS workers kept failing:\n{last_error}")


def test_rccl_journal_checkpoint_roundtrip(tmp_path) -> None:
    """RcclStorage <-> journal file: checkpoint and resume share the log format."""
    import datetime

    from torch.distributed import TCPStore

    import optuna_amd
    from optuna_amd.storages import JournalStorage
    from optuna_amd.storages._rccl import RcclStorage
    from optuna_amd.storages.journal import JournalFileBackend

    store = TCPStore("127.0.0.1", _free_port(), 1, is_master=True,
                     timeout=datetime.timedelta(seconds=30))
    storage = RcclStorage(store)
    study = optuna_amd.create_study(storage=storage, study_name="ckpt")
    study.optimize(lambda t: t.suggest_float("x", -1, 1) ** 2, n_trials=8)

    path = str(tmp_path / "ckpt.jsonl")
    storage.to_journal(JournalFileBackend(path))

    js = JournalStorage(JournalFileBackend(path))
    resumed = optuna_amd.load_study(study_name="ckpt", storage=js)
    assert len(resumed.trials) == 8
    assert resumed.best_value == study.best_value

    # Resume the journal into a fresh shared log.
    store2 = TCPStore("127.0.0.1", _free_port(), 1, is_master=True,
                      timeout=datetime.timedelta(seconds=30))
    storage2 = RcclStorage(store2)
    storage2.load_journal(JournalFileBackend(path))
    study2 = optuna_amd.load_study(study_name="ckpt", storage=storage2)
    assert len(study2.trials) == 8
    study2.optimize(lambda t: t.suggest_float("x", -1, 1) ** 2, n_trials=4)
    assert len(study2.trials) == 12

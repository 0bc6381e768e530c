"""End-to-end wire-protocol proxy tests: our wire client against our wire
server, then cross-compatibility against the REFERENCE's generated stubs
(their client classes driving our server) when the reference is available."""
from __future__ import annotations

import socket
import threading

import pytest

import optuna_amd
from optuna_amd.storages import InMemoryStorage
from optuna_amd.storages._grpc.wire_client import GrpcWireStorageProxy
from optuna_amd.storages._grpc.wire_server import make_wire_server
from optuna_amd.trial import TrialState


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def wire_pair():
    port = _free_port()
    backend = InMemoryStorage()
    server = make_wire_server(backend, "127.0.0.1", port)
    server.start()
    client = GrpcWireStorageProxy(host="127.0.0.1", port=port)
    client.wait_server_ready(timeout=20)
    yield client, backend
    client.close()
    server.stop(None)


def test_wire_proxy_end_to_end(wire_pair) -> None:
    client, _ = wire_pair
    study = optuna_amd.create_study(storage=client, study_name="wire")
    study.set_user_attr("team", {"a": 1})

    def obj(t):
        x = t.suggest_float("x", -1, 1)
        i = t.suggest_int("i", 1, 8)
        t.report(x, step=0)
        if t.number == 2:
            raise optuna_amd.TrialPruned()
        return x * x + i

    study.optimize(obj, n_trials=6)
    assert len(study.trials) == 6
    assert study.user_attrs == {"team": {"a": 1}}
    states = [t.state for t in study.trials]
    assert states.count(TrialState.PRUNED) == 1
    # reload via a second client
    c2 = GrpcWireStorageProxy(host=client._host, port=client._port)
    s2 = optuna_amd.load_study(study_name="wire", storage=c2)
    assert len(s2.trials) == 6
    assert s2.best_value == study.best_value
    c2.close()


def test_reference_stub_against_our_server(wire_pair) -> None:
    """The reference's generated protobuf classes drive our wire server.

    Always replayed from the request bytes those classes emitted when
    ``tests/golden/reference/grpc_wire.json`` was recorded; with a reference
    checkout at hand (OPTUNA_REFERENCE_PATH) its classes also drive the server
    live."""
    import grpc

    from test_grpc_wire import GOLDEN, _load_ref_pb2

    from optuna_amd.storages._grpc import _wire

    client, backend = wire_pair
    channel = grpc.insecure_channel(f"127.0.0.1:{client._port}")

    # The recorded requests name study 2 and trial 3: occupy the ids before them.
    for i in range(2):
        filler = backend.create_new_study([optuna_amd.study.StudyDirection.MINIMIZE], f"f{i}")
    for _ in range(3):
        backend.create_new_trial(filler)

    def raw_call(method: str) -> dict:
        call = channel.unary_unary(
            f"/optuna.StorageService/{method}",
            request_serializer=lambda b: b,
            response_deserializer=lambda b: b,
        )
        reply = call(bytes.fromhex(GOLDEN["stub_requests"][method]))
        return _wire.decode(_wire.METHODS[method][1], reply)

    assert raw_call("CreateNewStudy")["study_id"] == 2
    assert client.get_study_id_from_name("refstub") == 2
    assert raw_call("CreateNewTrial")["trial_id"] == 3
    replayed = raw_call("GetTrial")["trial"]
    assert replayed["trial_id"] == 3 and replayed["state"] == GOLDEN["enums"]["RUNNING"]
    assert client.get_trial(3).state == TrialState.RUNNING
    backend.delete_study(2)

    pb2 = _load_ref_pb2()
    if pb2 is None:
        channel.close()
        return
    call = channel.unary_unary(
        "/optuna.StorageService/CreateNewStudy",
        request_serializer=lambda m: m.SerializeToString(),
        response_deserializer=pb2.CreateNewStudyReply.FromString,
    )
    rep = call(pb2.CreateNewStudyRequest(directions=[pb2.MINIMIZE], study_name="refstub"))
    sid = rep.study_id

    call2 = channel.unary_unary(
        "/optuna.StorageService/CreateNewTrial",
        request_serializer=lambda m: m.SerializeToString(),
        response_deserializer=pb2.CreateNewTrialReply.FromString,
    )
    tid = call2(pb2.CreateNewTrialRequest(study_id=sid, template_trial_is_none=True)).trial_id

    call3 = channel.unary_unary(
        "/optuna.StorageService/GetTrial",
        request_serializer=lambda m: m.SerializeToString(),
        response_deserializer=pb2.GetTrialReply.FromString,
    )
    trial = call3(pb2.GetTrialRequest(trial_id=tid)).trial
    assert trial.trial_id == tid and trial.state == pb2.RUNNING
    # And our wire client sees the study made through the reference stubs.
    assert client.get_study_id_from_name("refstub") == sid
    channel.close()

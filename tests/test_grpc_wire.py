"""Wire-format oracle tests: our hand-written codec must produce bytes the
reference's generated protobuf classes parse (and vice versa), for every
message in api.proto.

The reference's side is replayed from ``tests/golden/reference/grpc_wire.json``
(recorded by ``scripts/record_reference_goldens.py``), so the tests run
anywhere; where a reference checkout is importable they also query it live."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import pytest

from optuna_amd.storages._grpc import _wire

GOLDEN = json.loads(
    (Path(__file__).parent / "golden" / "reference" / "grpc_wire.json").read_text()
)


def _load_ref_pb2():
    """The reference's generated module from the checkout that
    OPTUNA_REFERENCE_PATH names, or None when there is none to import."""
    root = os.environ.get("OPTUNA_REFERENCE_PATH")
    if not root:
        return None
    path = f"{root}/optuna/storages/_grpc/auto_generated"
    import importlib.util

    if not os.path.isdir(path):
        return None
    spec = importlib.util.spec_from_file_location("api_pb2", f"{path}/api_pb2.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["api_pb2"] = mod
    try:
        spec.loader.exec_module(mod)
    except Exception:  # protobuf runtime mismatch etc.
        return None
    return mod


def _jsonable(obj):
    # Same normalisation as the recorder: map keys become strings.
    return json.loads(json.dumps(obj))


SAMPLES = {
    "CreateNewStudy": (
        {"directions": [0, 1, 0], "study_name": "abc"},
        {"study_id": 42},
    ),
    "DeleteStudy": ({"study_id": 7}, {}),
    "SetStudyUserAttribute": ({"study_id": 1, "key": "k", "value": '"v"'}, {}),
    "SetStudySystemAttribute": ({"study_id": 1, "key": "k", "value": "1"}, {}),
    "GetStudyIdFromName": ({"study_name": "s"}, {"study_id": 3}),
    "GetStudyNameFromId": ({"study_id": 3}, {"study_name": "s"}),
    "GetStudyDirections": ({"study_id": 3}, {"directions": [1, 1]}),
    "GetStudyUserAttributes": ({"study_id": 3}, {"user_attributes": {"a": "1", "b": '"x"'}}),
    "GetStudySystemAttributes": ({"study_id": 3}, {"system_attributes": {"c": "2"}}),
    "GetAllStudies": (
        {},
        {
            "studies": [
                {
                    "study_id": 1,
                    "study_name": "n",
                    "directions": [0],
                    "user_attributes": {"u": "1"},
                    "system_attributes": {},
                }
            ]
        },
    ),
    "CreateNewTrial": (
        {
            "study_id": 2,
            "template_trial": {
                "trial_id": 0,
                "number": 0,
                "state": 1,
                "values": [0.5],
                "datetime_start": "2026-01-01T00:00:00",
                "datetime_complete": "2026-01-01T00:00:01",
                "params": {"x": 1.25},
                "distributions": {"x": "{}"},
                "user_attributes": {},
                "system_attributes": {},
                "intermediate_values": {1: 0.5, 2: -0.25},
            },
            "template_trial_is_none": False,
        },
        {"trial_id": 9},
    ),
    "SetTrialParameter": (
        {
            "trial_id": 1,
            "param_name": "x",
            "param_value_internal": -1.5,
            "distribution": '{"name": "FloatDistribution"}',
        },
        {},
    ),
    "GetTrialIdFromStudyIdTrialNumber": (
        {"study_id": 1, "trial_number": 4},
        {"trial_id": 11},
    ),
    "SetTrialStateValues": (
        {"trial_id": 1, "state": 2, "values": [1.0, 2.0]},
        {"trial_updated": True},
    ),
    "SetTrialIntermediateValue": (
        {"trial_id": 1, "step": 3, "intermediate_value": 0.75},
        {},
    ),
    "SetTrialUserAttribute": ({"trial_id": 1, "key": "k", "value": "null"}, {}),
    "SetTrialSystemAttribute": ({"trial_id": 1, "key": "k", "value": "[]"}, {}),
    "GetTrial": (
        {"trial_id": 1},
        {
            "trial": {
                "trial_id": 1,
                "number": 0,
                "state": 0,
                "values": [],
                "datetime_start": "",
                "datetime_complete": "",
                "params": {},
                "distributions": {},
                "user_attributes": {},
                "system_attributes": {},
                "intermediate_values": {},
            }
        },
    ),
    "GetTrials": (
        {"study_id": 1, "included_trial_ids": [1, 2, 9], "trial_id_greater_than": 5},
        {"trials": []},
    ),
}


def _msg_to_dict(schema, pb):
    out = {}
    for name, spec in schema.items():
        kind = spec[1]
        v = getattr(pb, name)
        if kind == "map":
            out[name] = dict(v)
        elif kind in ("rep_int64", "rep_double", "rep_enum"):
            out[name] = list(v)
        elif kind == "rep_msg":
            out[name] = [_msg_to_dict(spec[2], item) for item in v]
        elif kind == "msg":
            out[name] = _msg_to_dict(spec[2], v)
        elif kind == "bool":
            out[name] = bool(v)
        else:
            out[name] = v
    return out


@pytest.mark.parametrize("method", sorted(SAMPLES))
def test_wire_matches_reference_pb2(method) -> None:
    req_schema, rep_schema = _wire.METHODS[method]
    sides = (
        ("request", req_schema, SAMPLES[method][0], f"{method}Request"),
        ("reply", rep_schema, SAMPLES[method][1], f"{method}Reply"),
    )
    for side, schema, payload, _ in sides:
        golden = GOLDEN["messages"][method][side]
        ours = _wire.encode(schema, payload)
        # Our bytes are the ones the reference parsed when the fixture was
        # recorded, and it read the same content out of them as we do.
        assert ours.hex() == golden["ours_hex"]
        assert golden["reference_parse_of_ours"] == _jsonable(_wire.decode(schema, ours))
        # We parse the reference's own bytes to the same content.
        theirs = bytes.fromhex(golden["reference_hex"])
        assert _wire.decode(schema, theirs) == _wire.decode(schema, ours)

    pb2 = _load_ref_pb2()
    if pb2 is None:
        return
    for _, schema, payload, cls_name in sides:
        cls = getattr(pb2, cls_name)
        ours = _wire.encode(schema, payload)
        # Reference parses our bytes to the same content.
        ref_msg = cls.FromString(ours)
        assert _msg_to_dict(schema, ref_msg) == _wire.decode(schema, ours)
        # We parse the reference's bytes to the same content.
        theirs = ref_msg.SerializeToString()
        assert _wire.decode(schema, theirs) == _wire.decode(schema, ours)

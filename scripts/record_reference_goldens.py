"""Record the reference-interop fixtures under ``tests/golden/reference/``.

Usage: ``python scripts/record_reference_goldens.py --reference PATH`` where PATH
is a checkout of the reference library. The script runs the reference's own
code and stores only what it reads and writes: serialized protobuf messages,
its ORM table layout, a journal log it wrote and its distribution JSON. The
interop tests replay these files, so they need no reference checkout; when one
is present they additionally talk to it live.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import json
import logging
import os
import sys
import types
from pathlib import Path


REPO = Path(__file__).resolve().parent.parent
OUT = REPO / "tests" / "golden" / "reference"


def _install_colorlog_stub() -> None:
    # The reference hard-requires colorlog; a plain-formatter stand-in suffices.
    if "colorlog" in sys.modules:
        return
    try:
        import colorlog  # noqa: F401

        return
    except ImportError:
        pass
    stub = types.ModuleType("colorlog")

    class _Fmt(logging.Formatter):
        def __init__(self, fmt=None, **kwargs):
            if fmt:
                fmt = fmt.replace("%(log_color)s", "").replace("%(reset)s", "")
            super().__init__(fmt)

    stub.ColoredFormatter = _Fmt
    stub.TTYColoredFormatter = _Fmt
    stub.StreamHandler = logging.StreamHandler
    sys.modules["colorlog"] = stub


def _jsonable(obj):
    """Normalise through JSON (map keys become strings, tuples lists)."""
    return json.loads(json.dumps(obj))


def record_grpc_wire(reference: Path) -> None:
    from google.protobuf import json_format

    sys.path.insert(0, str(REPO / "tests"))
    from test_grpc_wire import SAMPLES, _msg_to_dict

    from optuna_amd.storages._grpc import _wire

    path = reference / "optuna" / "storages" / "_grpc" / "auto_generated" / "api_pb2.py"
    spec = importlib.util.spec_from_file_location("api_pb2", path)
    pb2 = importlib.util.module_from_spec(spec)
    sys.modules["api_pb2"] = pb2
    spec.loader.exec_module(pb2)

    messages = {}
    for method in sorted(SAMPLES):
        req_schema, rep_schema = _wire.METHODS[method]
        entry = {}
        for side, schema, payload, cls_name in (
            ("request", req_schema, SAMPLES[method][0], f"{method}Request"),
            ("reply", rep_schema, SAMPLES[method][1], f"{method}Reply"),
        ):
            cls = getattr(pb2, cls_name)
            ours = _wire.encode(schema, payload)
            parsed = cls.FromString(ours)
            built = json_format.ParseDict(_jsonable(payload), cls())
            entry[side] = {
                # our encoding at record time, and what the reference made of it
                "ours_hex": ours.hex(),
                "reference_parse_of_ours": _jsonable(_msg_to_dict(schema, parsed)),
                # the reference's own bytes for a message it built from the payload
                "reference_hex": built.SerializeToString(deterministic=True).hex(),
            }
        messages[method] = entry

    # Requests the reference's classes emit for the end-to-end stub test.
    stub = {
        "CreateNewStudy": pb2.CreateNewStudyRequest(
            directions=[pb2.MINIMIZE], study_name="refstub"
        ),
        "CreateNewTrial": pb2.CreateNewTrialRequest(study_id=2, template_trial_is_none=True),
        "GetTrial": pb2.GetTrialRequest(trial_id=3),
    }
    out = {
        "messages": messages,
        "stub_requests": {k: v.SerializeToString().hex() for k, v in stub.items()},
        "enums": {"MINIMIZE": pb2.MINIMIZE, "RUNNING": pb2.RUNNING},
    }
    (OUT / "grpc_wire.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


def record_rdb_models(reference_optuna) -> None:
    models = importlib.import_module("optuna.storages._rdb.models")
    tables = {}
    for name, table in sorted(models.BaseModel.metadata.tables.items()):
        cols = {}
        for c in table.columns:
            cols[c.name] = {
                "primary_key": bool(c.primary_key),
                "type": type(c.type).__name__,
                "enums": list(c.type.enums) if hasattr(c.type, "enums") else None,
            }
        tables[name] = cols
    dist = reference_optuna.distributions.FloatDistribution(-5.0, 5.0)
    out = {
        "schema_version": models.SCHEMA_VERSION,
        "tables": tables,
        "float_distribution_json": reference_optuna.distributions.distribution_to_json(dist),
    }
    (OUT / "rdb_models.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


def record_journal(reference_optuna) -> None:
    sys.path.insert(0, str(REPO / "tests"))
    from test_reference_compat import _populate

    path = OUT / "journal_interop.log"
    if path.exists():
        path.unlink()
    storage = reference_optuna.storages.JournalStorage(
        reference_optuna.storages.journal.JournalFileBackend(str(path))
    )
    _populate(reference_optuna, storage)
    for leftover in OUT.glob("journal_interop.log.*"):
        leftover.unlink()


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("--reference", required=True, help="reference checkout")
    args = parser.parse_args()
    reference = Path(args.reference).resolve()

    os.makedirs(OUT, exist_ok=True)
    sys.path.insert(0, str(REPO))
    record_grpc_wire(reference)

    _install_colorlog_stub()
    sys.path.insert(0, str(reference))
    import optuna as reference_optuna

    reference_optuna.logging.set_verbosity(reference_optuna.logging.WARNING)
    record_rdb_models(reference_optuna)
    record_journal(reference_optuna)


if __name__ == "__main__":
    main()

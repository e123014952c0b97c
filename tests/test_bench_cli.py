"""bench.py's command line: a plain run measures the timed loop alone, --full adds the reported extras (no GPU needed:
bench.py imports torch only inside main)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import bench as b
    return b


def parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_full_is_off_by_default(bench, monkeypatch):
    args = parse(bench, monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert args.full is False
    assert (args.gpus, args.steps, args.warmup, args.dump_outputs) == (1, 5, 2, None)
    assert parse(bench, monkeypatch, "--full").full is True


@pytest.mark.parametrize("argv, legs", [
    ((), (False, False)),                                   # plain: the timed loop alone
    (("--dump-outputs", "out"), (False, False)),
    (("--no-cpu-baseline",), (False, False)),
    (("--full",), (True, True)),
    (("--full", "--no-cpu-baseline"), (True, True)),        # the C++ API legs stay
    (("--only-roofline",), (True, False)),                  # the single-context passes alone
    (("--full", "--only-roofline"), (True, False)),
    (("--quick",), (False, False)),
    (("--quick", "--full"), (False, False)),
])
def test_which_extras_a_run_does(bench, monkeypatch, argv, legs):
    assert tuple(bool(x) for x in bench.extra_legs(parse(bench, monkeypatch, *argv))) == legs

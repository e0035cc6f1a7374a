"""tools/ab_bench.py, the child-process A/B method of the tools/bench_<feature>.py, driven with a stub child (no GPU, no renderer): the
order of the legs, what reaches a child, its environment, the arithmetic, the stop at the first failed leg, and each tool's own fields."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
with open(os.path.join(ROOT, "tests", "golden", "bench_tool_keys.json")) as f:
    TOOL_KEYS = json.load(f)  # recorded from the tools as they were before the harness, each fed canned child lines
COMMON_KEYS = ["leg", "loop", "size", "spp", "bounces", "frames", "rounds", "frame_ms_median", "round_medians_ms", "spread_ms"]

STUB = '''import json, os, sys
leg, log = sys.argv[sys.argv.index("--leg") + 1], os.environ["STUB_LOG"]
with open(log, "a") as f:
    f.write(json.dumps({"argv": sys.argv[1:], "lib": os.environ.get("WFPT_LIB", "unset")}) + "\\n")
with open(log) as f:
    n = sum(json.loads(line)["argv"][1] == leg for line in f)
if leg == "boom":
    sys.exit(3)
print("not the last line")
print(json.dumps(json.load(open(os.environ["STUB_CANNED"]))[leg][n - 1]))
'''


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def ab(monkeypatch):
    monkeypatch.syspath_prepend(TOOLS)  # (a tool run as a script has its own folder there)
    monkeypatch.delitem(sys.modules, "ab_bench", raising=False)
    return load("ab_bench")


@pytest.fixture
def stub(tmp_path, monkeypatch):
    """(script, log reader, canned writer): the child appends to the log and answers with canned[leg][its call count - 1]"""
    script, log, canned = tmp_path / "bench_stub.py", tmp_path / "log.jsonl", tmp_path / "canned.json"
    script.write_text(STUB)
    monkeypatch.setenv("STUB_LOG", str(log))
    monkeypatch.setenv("STUB_CANNED", str(canned))
    monkeypatch.setenv("WFPT_LIB", "/x")

    def calls():
        return [json.loads(line) for line in log.read_text().splitlines()] if log.exists() else []

    def options(argv):  # argv as {option: value}; --leg and --tree lead, the rest in pairs
        return dict(zip(argv[0::2], argv[1::2]))

    return str(script), calls, lambda d: canned.write_text(json.dumps(d)), options


def child_line(leg, frames, **extra):
    return {"leg": leg, "loop": "refill", "frame_ms": frames, **extra}


def test_order_forwarding_and_environment(ab, stub, tmp_path, capsys):
    script, calls, can, options = stub
    ap = ab.parser(frames=12)
    ap.add_argument("--room-bounces", type=int, default=50)  # an option of the tool's own
    ap.add_argument("--equal-time", type=float, default=0.0)
    for orchestration in ("--scenes", "--legs"):
        ap.add_argument(orchestration, nargs="+", default=["a", "b"])
    for orchestration in ("--parent-tree", "--parent-root", "--closest-lib"):
        ap.add_argument(orchestration, default=None)
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args(["--rounds", "2", "--width", "64", "--equal-time", "7.5", "--parent-tree", "/p", "--closest-lib", "/c", "--no-quality"])
    lib = str(tmp_path / "libclosest.so")
    legs = [ab.entry("A"), ab.entry("B@parent", tree=str(tmp_path), equal_time=0.0), ab.entry("C@closest", lib=lib)]
    can({name: [child_line(name, [1.0])] * 2 for name in "ABC"})
    results = ab.run_legs(script, legs, args)
    assert list(results) == ["A", "B@parent", "C@closest"] and all(len(r) == 2 for r in results.values())
    seen = calls()
    assert [c["argv"][:4] for c in seen] == [["--leg", "A", "--tree", ab.ROOT], ["--leg", "B", "--tree", str(tmp_path)],
                                             ["--leg", "C", "--tree", ab.ROOT]] * 2
    forwarded = {"--width": "64", "--height": "1080", "--spp": "64", "--bounces": "8", "--frames": "12", "--triangles": "1000000",
                 "--room-bounces": "50", "--equal-time": "7.5"}
    for c in seen:
        leg = c["argv"][1]
        assert options(c["argv"][4:]) == ({**forwarded, "--equal-time": "0.0"} if leg == "B" else forwarded)  # the override, for B alone
        assert c["lib"] == (lib if leg == "C" else "unset")  # never the parent's /x
    assert capsys.readouterr().err.splitlines() == ["A: 1.000 ms", "B@parent: 1.000 ms", "C@closest: 1.000 ms"] * 2


def test_arithmetic_rounding_and_key_order(ab, stub, capsys):
    script, _, can, _ = stub
    args = ab.parser(frames=3).parse_args(["--rounds", "2", "--bounces", "8"])
    can({"A": [child_line("A", [4, 2, 9], n=7, f=1.23456789, skipped=1.5, late=0.1234567),
               child_line("A", [1, 8, 3], n=8, f=2.3456789, skipped=1.5)],
         "room": [child_line("room", [5.0, 6.0])] * 2})
    results = ab.run_legs(script, [ab.entry("A"), ab.entry("room")], args)
    summary = ab.summarise(results, args, ("f", "n", "late"), 4, bounces_of=lambda name: 50 if name == "room" else args.bounces)
    line = summary["A"]
    assert (line["frame_ms_median"], line["round_medians_ms"], line["spread_ms"]) == (3.5, [4, 3], 1.0)
    assert list(line) == COMMON_KEYS + ["f", "n"]  # the extras in the order asked for, from the last round's child, what it lacks left out
    assert line["f"] == 2.3457 and line["n"] == 8 and isinstance(line["n"], int)
    assert (line["loop"], line["size"], line["spp"], line["bounces"], line["frames"], line["rounds"]) == ("refill", [1920, 1080], 64, 8, 3, 2)
    assert summary["room"]["bounces"] == 50 and list(summary["room"]) == COMMON_KEYS
    assert ab.summarise(results, args, ("f",), None)["A"]["f"] == 2.3456789  # no digits: as it came
    assert [json.loads(x) for x in capsys.readouterr().out.splitlines()][:2] == [summary["A"], summary["room"]]  # one line per leg


def test_ratios(ab):
    summary = {"a": {"frame_ms_median": 3.0, "v": 1.0}, "b": {"frame_ms_median": 7.0, "v": 4.0}}
    assert ab.ratios(summary, [("a", "b"), ("a", "gone"), ("gone", "b"), ("b", "a")]) == {"a over b": round(3.0 / 7.0 - 1, 4), "b over a": round(7.0 / 3.0 - 1, 4)}
    assert ab.ratios(summary, [("b", "a")], ", frame") == {"b over a, frame": 1.3333}
    assert ab.ratios(summary, [("b", "a")], ", v", "v") == {"b over a, v": 3.0}
    assert ab.twin_pairs({"a": 0, "a@parent": 0, "b": 0}) == [("a", "a@parent"), ("b", "b@parent")]


def test_a_failed_leg_ends_the_run(ab, stub):
    """No child is started after one that failed: what keeps a faulted leg from being followed by more work on the device."""
    script, calls, can, _ = stub
    can({name: [child_line(name, [1.0])] * 2 for name in "AC"})
    args = ab.parser().parse_args(["--rounds", "2"])
    with pytest.raises(SystemExit) as e:
        ab.run_legs(script, [ab.entry("A"), ab.entry("boom"), ab.entry("C")], args)
    assert str(e.value) == "bench_stub: leg boom failed with status 3"
    assert [c["argv"][1] for c in calls()] == ["A", "boom"]


def test_with_twins(ab):
    legs = [ab.entry("x:a"), ab.entry("x:b")]
    assert ab.with_twins(legs, None) == legs
    twinned = ab.with_twins(legs, "/p", lambda name: name.endswith("a"))
    assert [(l[0], l[1], l[2]) for l in twinned] == [("x:a", "x:a", ab.ROOT), ("x:a@parent", "x:a", "/p"), ("x:b", "x:b", ab.ROOT)]


@pytest.mark.parametrize("tool", sorted(TOOL_KEYS))
def test_each_tool_keeps_its_legs_and_fields(ab, tool, monkeypatch):
    want = TOOL_KEYS[tool]
    monkeypatch.delitem(sys.modules, "wavefront_path_tracer_amd", raising=False)
    mod = load(tool)
    assert "wavefront_path_tracer_amd" not in sys.modules  # the parent role needs no renderer
    args = mod.options().parse_args(want["argv"])
    legs = mod.legs(args)
    assert [leg[0] for leg in legs] == want["legs"] and mod.DIGITS == want["digits"]
    extras = want["keys"][len(COMMON_KEYS):]
    child = child_line("x", [1.0, 2.0], **{k: 1.23456789 for k in reversed(extras)}, frame=0, unknown=1)
    line = ab.summarise({leg[0]: [child] for leg in legs}, args, mod.EXTRA_KEYS, mod.DIGITS)[want["legs"][-1]]
    assert list(line) == want["keys"]
    assert line[extras[0]] == (1.23456789 if want["digits"] is None else round(1.23456789, want["digits"]))

"""ganslate_amd/switches.py is the one place that declares and reads the GS_* switches: nothing else in the package reads
one from the environment, every name a test sets is declared, an undeclared name raises, and the accessors read the
environment at the moment of the call."""
import re
from pathlib import Path

import pytest

from ganslate_amd import switches

ROOT = Path(__file__).resolve().parent.parent
# os.environ.get("GS_TWIN" ... / os.environ["GS_TWIN"] / os.getenv("GS_TWIN" ... / "GS_TWIN" in os.environ. The pattern sees
# names written out at the read; it would miss `from os import environ` and a computed name (neither occurs in the package).
ENV_READ = re.compile(r"""(?:os\.environ(?:\.get\(|\[|\.pop\(|\.setdefault\()|os\.getenv\()\s*f?["']GS_\w*|["']GS_\w+["']\s+(?:not\s+)?in\s+os\.environ""")
# Tests hand names to monkeypatch.setenv directly, through parametrize lists and through dicts: every quoted GS_* literal
# under tests/ is taken for a switch name unless it is one of the C header's constants.
GS_LITERAL = re.compile(r"""["'](GS_[A-Z0-9_]+)["']""")
ABI_CONSTANTS = {"GS_MAX_TAPS", "GS_BORDER_REFLECT", "GS_BORDER_REPLICATE", "GS_ACT_RELU", "GS_ACT_LRELU", "GS_ACT_TANH",
                 "GS_OPTIONS"}


def declared(name):
    return name in switches.HOST_SWITCHES or name in switches.LIBRARY_OPTIONS.values()


def test_only_switches_py_reads_a_gs_variable():
    hits = []
    for path in sorted((ROOT / "ganslate_amd").rglob("*.py")):
        if path.name == "switches.py" and path.parent.name == "ganslate_amd":
            continue
        for n, line in enumerate(path.read_text().splitlines(), 1):
            if ENV_READ.search(line):
                hits.append(f"{path.relative_to(ROOT)}:{n}: {line.strip()}")
    assert not hits, "GS_* variables are read through ganslate_amd.switches only:\n" + "\n".join(hits)


def test_the_read_pattern_finds_the_forms_it_is_meant_to():
    for line in ('os.environ.get("GS_TWIN", "1") == "0"', "os.environ['GS_TWIN']", 'os.getenv("GS_TWIN")', 'if "GS_TWIN" in os.environ:',
                 'os.environ.get( "GS_TWIN")'):
        assert ENV_READ.search(line), line
    for line in ('os.environ.get("WORLD_SIZE", 1)', 'switches.on("GS_TWIN")', 'os.environ.get("GANSLATE_HIP_LIB")'):
        assert not ENV_READ.search(line), line


def test_every_switch_a_test_sets_is_declared():
    seen = set()
    for path in sorted((ROOT / "tests").rglob("*.py")):
        if path.name == "test_switches_cpu.py":      # (its own examples are not evidence)
            continue
        for name in set(GS_LITERAL.findall(path.read_text())) - ABI_CONSTANTS:
            seen.add(name)
            assert declared(name), f"{path.relative_to(ROOT)} names {name}, which ganslate_amd/switches.py does not declare"
    # the scan does find them: names only a parametrize list of test_gradients_gpu.py holds, a library variable, free-form ones
    assert {"GS_WGRAD_PAIR", "GS_FUSE_NORM", "GS_HCONVW_RING", "GS_HWGRAD_FT", "GS_TWIN", "GS_DDP_GRAPH_COLLECTIVES"} <= seen
    assert declared("GS_SIDE_STREAM") and declared("GS_FORCE_DDP")     # (bench.py sets these two itself)


def test_tables_are_consistent():
    kinds = {switches.ON_OFF, switches.OPT_IN, switches.INT, switches.STR}
    for name, (default, kind, meaning) in switches.HOST_SWITCHES.items():
        assert name.startswith("GS_") and kind in kinds and meaning, name
        assert default is None or isinstance(default, str), name
        if kind in (switches.ON_OFF, switches.OPT_IN):
            assert default in ("0", "1"), name
    both = set(switches.HOST_SWITCHES) & set(switches.LIBRARY_OPTIONS.values())
    assert both == {"GS_HWGRAD_PLANES"}, "the only variable that is a library option AND read by the host"
    assert switches.LIBRARY_OPTIONS["hconv5_seg"] is None


def test_an_undeclared_name_raises(monkeypatch):
    bogus = "GS_" + "NO_SUCH_SWITCH"
    monkeypatch.setenv(bogus, "1")
    for read in (switches.on, switches.value, switches.raw):
        with pytest.raises(KeyError):
            read(bogus)
    with pytest.raises(KeyError):
        switches.on("GS_SPLITK")            # a library option is not a host switch: the library is asked, not the environment
    with pytest.raises(KeyError):
        switches.library_value("no_such_option")
    assert not declared(bogus)


def test_accessors_read_the_environment_at_the_call(monkeypatch):
    monkeypatch.delenv("GS_FUSE_NORM", raising=False)
    assert switches.on("GS_FUSE_NORM") and switches.value("GS_FUSE_NORM") is True
    monkeypatch.setenv("GS_FUSE_NORM", "0")
    assert not switches.on("GS_FUSE_NORM")
    monkeypatch.setenv("GS_FUSE_NORM", "2")          # on/off: off if and only if "0"
    assert switches.on("GS_FUSE_NORM")
    monkeypatch.delenv("GS_FORCE_DDP", raising=False)
    assert not switches.on("GS_FORCE_DDP")
    monkeypatch.setenv("GS_FORCE_DDP", "2")          # opt-in: on if and only if "1"
    assert not switches.on("GS_FORCE_DDP")
    monkeypatch.setenv("GS_FORCE_DDP", "1")
    assert switches.on("GS_FORCE_DDP")
    monkeypatch.delenv("GS_TWIN", raising=False)
    assert switches.raw("GS_TWIN") == "1"
    monkeypatch.setenv("GS_TWIN", "2d")
    assert switches.raw("GS_TWIN") == switches.value("GS_TWIN") == "2d"
    monkeypatch.delenv("GS_DDP_GRAPH_COLLECTIVES", raising=False)
    assert switches.raw("GS_DDP_GRAPH_COLLECTIVES", "auto") == "auto" and switches.raw("GS_DDP_GRAPH_COLLECTIVES") is None
    monkeypatch.setenv("GS_DDP_GRAPH_COLLECTIVES", "1")
    assert switches.raw("GS_DDP_GRAPH_COLLECTIVES", "auto") == "1"
    monkeypatch.delenv("GS_EARLY_ADAM_MIN", raising=False)
    assert switches.value("GS_EARLY_ADAM_MIN", 1 << 21) == 1 << 21
    monkeypatch.setenv("GS_EARLY_ADAM_MIN", "4096")
    assert switches.value("GS_EARLY_ADAM_MIN", 1 << 21) == 4096
    monkeypatch.delenv("GS_HCONVT", raising=False)
    assert switches.library_value("hconvt") is None and switches.library_value("hconv5_seg") is None
    monkeypatch.setenv("GS_HCONVT", "0")
    assert switches.library_value("hconvt") == 0


def test_switches_module_stands_alone():
    """no import of the package or of torch: tools and CPU tests load it on its own"""
    src = (ROOT / "ganslate_amd" / "switches.py").read_text()
    imports = re.findall(r"^\s*(?:import|from)\s+(\S+)", src, flags=re.M)
    assert imports == ["os"], imports

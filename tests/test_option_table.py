"""The engine's options live in ONE table (kOptions, fastdem_amd/csrc/fdm_engine_opts.inl).  Plain file parsing, no GPU
and no library: the option list in include/fdm_engine.h names exactly the table's options, every table row stores into
a field of its own of struct EngineOptions, and every option name the benchmark, the tests, the Python package and the
C++ mirror pass to set_option is in the table."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastdem_amd", "csrc")


def _read(*parts):
    return open(os.path.join(*parts), errors="ignore").read()


def table_rows():
    """(name, field or None) per row of kOptions, in table order."""
    src = _read(CSRC, "fdm_engine_opts.inl")
    body = src[src.index("static const OptionRow kOptions[] = {"):]
    body = body[:body.index("\n};")]
    rows = re.findall(r'^\s*\{"(\w+)",\s*(?:&EngineOptions::(\w+)|nullptr),', body, flags=re.M)
    assert len(rows) == len(re.findall(r'^\s*\{"', body, flags=re.M)), "a row the parser does not understand"
    return [(name, field or None) for name, field in rows]


def header_names():
    """The quoted names of the option list in include/fdm_engine.h (the comment ahead of fdm_engine_set_option)."""
    src = _read(ROOT, "include", "fdm_engine.h")
    end = src.index("int fdm_engine_set_option(")
    comment = src[src.rindex("/*", 0, end):end]
    return re.findall(r'"(\w+)"', comment)


def option_fields():
    src = _read(CSRC, "fdm_engine_host.hpp")
    body = src[src.index("struct EngineOptions {"):]
    body = body[:body.index("\n};")]
    return re.findall(r"^  int (\w+) = ", body, flags=re.M)


def test_table_has_no_duplicates():
    names = [n for n, _ in table_rows()]
    assert names and len(set(names)) == len(names), names


def test_header_lists_exactly_the_table_in_table_order():
    names = [n for n, _ in table_rows()]
    listed = header_names()
    assert set(listed) == set(names), sorted(set(listed) ^ set(names))
    assert listed == names, [(a, b) for a, b in zip(listed, names) if a != b]


def test_every_option_field_has_exactly_one_row():
    fields = option_fields()
    stored = [f for _, f in table_rows() if f]
    assert sorted(stored) == sorted(fields), sorted(set(stored) ^ set(fields))
    assert len(set(stored)) == len(stored)
    assert [f for f in stored] == fields, "the table follows the order of EngineOptions' fields"
    for name, field in table_rows():
        assert field in (None, name), (name, field)


def test_engine_holds_no_option_outside_the_struct():
    src = _read(CSRC, "fdm_engine_host.hpp")
    engine = src[src.index("struct fdm_engine {"):]
    engine = engine[:engine.index("\n};")]
    assert "EngineOptions opt;" in engine
    for field in option_fields():
        assert not re.search(r"^  (?:bool|int|unsigned) %s\b" % field, engine, flags=re.M), field


def _names_passed(text):
    # a string literal as the first argument, or as the second behind the engine handle of the C call
    return set(re.findall(r'set_option\(\s*(?:[^,"()]+(?:\([^()]*\))?\s*,\s*)?"(\w+)"', text))


def test_every_name_the_callers_pass_is_in_the_table():
    files = [os.path.join(ROOT, "bench.py")]
    files += glob.glob(os.path.join(ROOT, "tests", "*.py"))
    files += glob.glob(os.path.join(ROOT, "fastdem_amd", "*.py"))
    for d, _, names in os.walk(os.path.join(ROOT, "fastdem_amd", "cpp")):
        files += [os.path.join(d, n) for n in names if n.endswith((".hpp", ".h", ".cpp", ".py", ".txt"))]
    known = {n for n, _ in table_rows()}
    passed = {}
    for f in files:
        for name in _names_passed(_read(f)):
            passed.setdefault(name, os.path.relpath(f, ROOT))
    assert {"overlap", "move_clear_basic", "voxel_any_order"} <= set(passed), sorted(passed)  # (bench.py, the tests, the C++ mirror)
    unknown = {n: f for n, f in passed.items() if n not in known}
    assert not unknown, unknown

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


def _caller_files(scripts=False):
    files = [os.path.join(ROOT, "bench.py")]
    files += glob.glob(os.path.join(ROOT, "tests", "*.py"))
    files += glob.glob(os.path.join(ROOT, "fastdem_amd", "*.py"))
    for d, _, names in os.walk(os.path.join(ROOT, "fastdem_amd", "cpp")):
        files += [os.path.join(d, n) for n in names if n.endswith((".hpp", ".h", ".cpp", ".py", ".txt"))]
    if scripts:
        files += glob.glob(os.path.join(ROOT, "scripts", "*.py"))
    return files


# Retired with the code only they reached (LABNOTES.md, "Retired: the stencil debug bits and sixteen unset options").
RETIRED = ("dbg_post", "bin_table", "borrow_inputs", "sync_spin_us", "upd_blocks", "upd_blocks_alone", "upd_prio",
           "tiled_lds_pad", "cnt_shift", "bin_delay", "bin_delay_blocks", "bin_stagger", "batch_ray_words", "ray_hold",
           "ray_wedge_parts", "dbg_no_atomics", "dbg_upd")


def _names_set(text):
    """Names a file sets: a literal handed to set_option, `key=value` inside a string (the `--set` switch of bench.py and
    the scripts), or — in a file that hands set_option a variable key — a quoted dictionary key with an integer value."""
    names = _names_passed(text)
    names |= set(re.findall(r'''["',](\w+)=-?\d''', text))
    if re.search(r"set_option\(\s*[A-Za-z_]\w*\s*,", text):
        names |= set(re.findall(r'"(\w+)":\s*-?\d', text))
    return names


def test_every_option_of_the_table_is_set_by_some_caller():
    """A row nobody sets is code nobody runs: the benchmark, a test, the package, the C++ mirror or a script under
    scripts/ sets every option of the table at least once."""
    this = os.path.abspath(__file__)
    used = set()
    for f in _caller_files(scripts=True):
        if os.path.abspath(f) != this:
            used |= _names_set(_read(f))
    unset = [n for n, _ in table_rows() if n not in used]
    assert not unset, unset
    assert not set(RETIRED) & {n for n, _ in table_rows()}


def test_retired_names_are_gone_from_the_sources():
    assert len(set(RETIRED)) == 17
    files = glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(ROOT, "include", "*"))
    assert len(files) > 40
    word = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    found = {os.path.relpath(f, ROOT): sorted(set(word.findall(_read(f)))) for f in files if os.path.isfile(f)}
    found = {f: names for f, names in found.items() if names}
    assert not found, found


def test_every_name_the_callers_pass_is_in_the_table():
    files = _caller_files()
    known = {n for n, _ in table_rows()}
    passed = {}
    for f in files:
        for name in _names_passed(_read(f)):
            passed.setdefault(name, os.path.relpath(f, ROOT))
    assert {"overlap", "move_clear_basic", "voxel_any_order"} <= set(passed), sorted(passed)  # (bench.py, the tests, the C++ mirror)
    unknown = {n: f for n, f in passed.items() if n not in known}
    assert not unknown, unknown

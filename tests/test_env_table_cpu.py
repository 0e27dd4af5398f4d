"""The library's environment switches (csrc/env.h, csrc/env.cpp): the parse rule
and the default of every row, the rule for "unset", and reload.  The env unit is
plain C++: it is compiled here with a small main of its own under
AddressSanitizer + UBSan and run as an ordinary executable, once per
environment; the expectations are written out by hand from the rules that
INTEGRATION.md and env.h state.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ucsa_neural_rendering_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "env.h"

static void show(const char* tag, const UcsaEnv& e) {
  printf("%s enc_sorted=%d\n", tag, (int)e.enc_sorted);
  printf("%s enc_ml=%d\n", tag, (int)e.enc_ml);
  printf("%s enc_sorted_ml=%u\n", tag, (unsigned)e.enc_sorted_ml);
  printf("%s density_fused=%d\n", tag, (int)e.density_fused);
  printf("%s density_levels=%u\n", tag, (unsigned)e.density_levels);
  printf("%s shade_bwd_split=%d\n", tag, (int)e.shade_bwd_split);
  printf("%s bwd_overlap=%d\n", tag, (int)e.bwd_overlap);
  printf("%s bwd_bin_scale=%.9g\n", tag, (double)e.bwd_bin_scale);
  printf("%s enc_order=%d:%s\n", tag, (int)e.enc_order.present, e.enc_order.value);
  printf("%s enc_simple=%u\n", tag, (unsigned)e.enc_simple);
  printf("%s enc_simple_h=%u\n", tag, (unsigned)e.enc_simple_h);
  printf("%s enc_simple_rays=%u\n", tag, (unsigned)e.enc_simple_rays);
  printf("%s sort_exact=%d\n", tag, (int)e.sort_exact);
  printf("%s components_no_lds=%d\n", tag, (int)e.components_no_lds);
}

// no argument: print the snapshot.  NAME=VALUE / NAME arguments: hold a reference
// to the snapshot, set / unset those variables, reload, then print what the held
// reference reads ("held") and what the new snapshot reads ("now").
int main(int argc, char** argv) {
  const UcsaEnv& first = ucsa_env();
  if (argc == 1) {
    show("now", first);
    return 0;
  }
  for (int i = 1; i < argc; ++i) {
    char* eq = strchr(argv[i], '=');
    if (eq) {
      *eq = 0;
      setenv(argv[i], eq + 1, 1);
    } else {
      unsetenv(argv[i]);
    }
  }
  ucsa_env_reload();
  const UcsaEnv& second = ucsa_env();
  show("held", first);
  show("now", second);
  printf("same_object=%d\n", (int)(&first == &second));
  ucsa_env_reload();   // a third snapshot: the first two still read the same
  show("held2", first);
  show("now2", second);
  return 0;
}
"""

DEFAULTS = {
    "enc_sorted": "2", "enc_ml": "-1", "enc_sorted_ml": "9", "density_fused": "1",
    "density_levels": "12", "shade_bwd_split": "1", "bwd_overlap": "1",
    "bwd_bin_scale": "100", "enc_order": "0:", "enc_simple": "16", "enc_simple_h": "0",
    "enc_simple_rays": "0", "sort_exact": "1", "components_no_lds": "0",
}
FIELD_OF = {
    "UCSA_ENC_SORTED": "enc_sorted", "UCSA_ENC_ML": "enc_ml",
    "UCSA_ENC_SORTED_ML": "enc_sorted_ml", "UCSA_DENSITY_FUSED": "density_fused",
    "UCSA_DENSITY_LEVELS": "density_levels", "UCSA_SHADE_BWD_SPLIT": "shade_bwd_split",
    "UCSA_BWD_OVERLAP": "bwd_overlap", "UCSA_BWD_BIN_SCALE": "bwd_bin_scale",
    "UCSA_ENC_ORDER": "enc_order", "UCSA_ENC_SIMPLE": "enc_simple",
    "UCSA_ENC_SIMPLE_H": "enc_simple_h", "UCSA_ENC_SIMPLE_RAYS": "enc_simple_rays",
    "UCSA_SORT_EXACT": "sort_exact", "UCSA_COMPONENTS_NO_LDS": "components_no_lds",
}
ON_UNLESS_0 = ("UCSA_DENSITY_FUSED", "UCSA_SHADE_BWD_SPLIT", "UCSA_BWD_OVERLAP",
               "UCSA_SORT_EXACT")
UNSIGNED = ("UCSA_ENC_SORTED_ML", "UCSA_ENC_SIMPLE", "UCSA_ENC_SIMPLE_H",
            "UCSA_ENC_SIMPLE_RAYS")

# (variable, value, what its field must read): a valid value and the edges of each rule
CASES = [
    # first character '0'..'4' -> that digit, else the default 2
    ("UCSA_ENC_SORTED", "0", "0"), ("UCSA_ENC_SORTED", "1", "1"), ("UCSA_ENC_SORTED", "3", "3"),
    ("UCSA_ENC_SORTED", "4", "4"), ("UCSA_ENC_SORTED", "5", "2"), ("UCSA_ENC_SORTED", "2x", "2"),
    ("UCSA_ENC_SORTED", "3x", "3"), ("UCSA_ENC_SORTED", "x3", "2"), ("UCSA_ENC_SORTED", "-1", "2"),
    # strtol; negative = no override (the consumer tests >= 0)
    ("UCSA_ENC_ML", "7", "7"), ("UCSA_ENC_ML", "0", "0"), ("UCSA_ENC_ML", "-1", "-1"),
    ("UCSA_ENC_ML", "-5", "-5"), ("UCSA_ENC_ML", "12abc", "12"), ("UCSA_ENC_ML", "abc", "0"),
    # atoi, then >= 16 -> 16, >= 12 -> 12, else 8
    ("UCSA_DENSITY_LEVELS", "8", "8"), ("UCSA_DENSITY_LEVELS", "11", "8"),
    ("UCSA_DENSITY_LEVELS", "12", "12"), ("UCSA_DENSITY_LEVELS", "15", "12"),
    ("UCSA_DENSITY_LEVELS", "16", "16"), ("UCSA_DENSITY_LEVELS", "99", "16"),
    ("UCSA_DENSITY_LEVELS", "0", "8"), ("UCSA_DENSITY_LEVELS", "-3", "8"),
    ("UCSA_DENSITY_LEVELS", "abc", "8"),
    # atof
    ("UCSA_BWD_BIN_SCALE", "60", "60"), ("UCSA_BWD_BIN_SCALE", "1e9", "1e+09"),
    ("UCSA_BWD_BIN_SCALE", "0", "0"), ("UCSA_BWD_BIN_SCALE", "160.5", "160.5"),
    # on iff the first character is '1'
    ("UCSA_COMPONENTS_NO_LDS", "0", "0"), ("UCSA_COMPONENTS_NO_LDS", "1", "1"),
    ("UCSA_COMPONENTS_NO_LDS", "2", "0"), ("UCSA_COMPONENTS_NO_LDS", "yes", "0"),
    ("UCSA_COMPONENTS_NO_LDS", "10", "1"),
    # text + "present"
    ("UCSA_ENC_ORDER", "2:0,1", "1:2:0,1"), ("UCSA_ENC_ORDER", "x", "1:x"),
]
for _name in ON_UNLESS_0:   # on unless the first character is '0'
    CASES += [(_name, "0", "0"), (_name, "1", "1"), (_name, "00", "0"), (_name, "01", "0"),
              (_name, "off", "1"), (_name, "10", "1")]
for _name in UNSIGNED:      # strtoul
    CASES += [(_name, "3", "3"), (_name, "0", "0"), (_name, "16", "16"), (_name, "7x", "7"),
              (_name, "x", "0")]

# a 64-character value that WOULD parse to something else than the default counts as
# unset; the same with 63 characters is taken
LONG = {
    "UCSA_ENC_SORTED": ("3" + "0" * 63, "3" + "0" * 62, "3"),
    "UCSA_ENC_ML": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_ENC_SORTED_ML": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_DENSITY_FUSED": ("0" * 64, "0" * 63, "0"),
    "UCSA_DENSITY_LEVELS": ("0" * 62 + "16", "0" * 61 + "16", "16"),
    "UCSA_SHADE_BWD_SPLIT": ("0" * 64, "0" * 63, "0"),
    "UCSA_BWD_OVERLAP": ("0" * 64, "0" * 63, "0"),
    "UCSA_BWD_BIN_SCALE": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_ENC_ORDER": ("1:" + "0" * 62, "1:" + "0" * 61, "1:1:" + "0" * 61),
    "UCSA_ENC_SIMPLE": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_ENC_SIMPLE_H": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_ENC_SIMPLE_RAYS": ("0" * 63 + "5", "0" * 62 + "5", "5"),
    "UCSA_SORT_EXACT": ("0" * 64, "0" * 63, "0"),
    "UCSA_COMPONENTS_NO_LDS": ("1" * 64, "1" * 63, "1"),
}


@pytest.fixture(scope="module")
def env_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_table")
    main = d / "env_main.cpp"
    main.write_text(MAIN)
    exe = d / "env_main"
    res = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",   # the runtimes inside the executable
         "-I", CSRC, "-I", os.path.join(ROOT, "include"),
         os.path.join(CSRC, "env.cpp"), str(main), "-o", str(exe), "-pthread"],
        capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def run(exe, env, *args):
    """{tag: {field: text}} of one run under exactly the UCSA_* variables of `env`"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("UCSA_")}
    res = subprocess.run([exe, *args], env={**base, **env}, capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, (env, args, res.returncode, res.stderr)
    out = {}
    for line in res.stdout.splitlines():
        if line.startswith("same_object="):
            out["same_object"] = line.split("=", 1)[1]
            continue
        tag, rest = line.split(" ", 1)
        field, value = rest.split("=", 1)
        out.setdefault(tag, {})[field] = value
    return out


def test_the_table_has_the_fourteen_rows_this_test_covers():
    import re
    rows = re.findall(r'X\("(UCSA_[A-Z0-9_]+)",\s*\w+,\s*(\w+),', open(os.path.join(CSRC, "env.h")).read())
    assert dict(rows) == FIELD_OF
    assert set(LONG) == set(FIELD_OF) and {c[0] for c in CASES} == set(FIELD_OF)


def test_unset_and_empty_give_every_default(env_exe):
    assert run(env_exe, {})["now"] == DEFAULTS
    assert run(env_exe, {name: "" for name in FIELD_OF})["now"] == DEFAULTS
    for name in FIELD_OF:    # one at a time too
        assert run(env_exe, {name: ""})["now"] == DEFAULTS, name


def test_a_value_of_64_characters_counts_as_unset_and_63_are_taken(env_exe):
    for name, (v64, v63, want63) in LONG.items():
        assert len(v64) == 64 and len(v63) == 63
        assert run(env_exe, {name: v64})["now"] == DEFAULTS, name
        assert run(env_exe, {name: v63})["now"] == {**DEFAULTS, FIELD_OF[name]: want63}, name
    assert run(env_exe, {name: v[0] for name, v in LONG.items()})["now"] == DEFAULTS
    assert run(env_exe, {name: "7" * 500 for name in FIELD_OF})["now"] == DEFAULTS


@pytest.mark.parametrize("name", sorted(FIELD_OF))
def test_parse_rule_valid_values_and_edges(env_exe, name):
    """Each value alone: its own field reads what the rule gives and every other field
    keeps its default (no row reads another row's variable)."""
    cases = [c for c in CASES if c[0] == name]
    assert cases
    for _, value, want in cases:
        got = run(env_exe, {name: value})["now"]
        assert got == {**DEFAULTS, FIELD_OF[name]: want}, (name, value)


def test_all_switches_at_once(env_exe):
    env = {"UCSA_ENC_SORTED": "4", "UCSA_ENC_ML": "3", "UCSA_ENC_SORTED_ML": "11",
           "UCSA_DENSITY_FUSED": "0", "UCSA_DENSITY_LEVELS": "16", "UCSA_SHADE_BWD_SPLIT": "0",
           "UCSA_BWD_OVERLAP": "0", "UCSA_BWD_BIN_SCALE": "1e9", "UCSA_ENC_ORDER": "1:3,2,1,0",
           "UCSA_ENC_SIMPLE": "1", "UCSA_ENC_SIMPLE_H": "2", "UCSA_ENC_SIMPLE_RAYS": "3",
           "UCSA_SORT_EXACT": "0", "UCSA_COMPONENTS_NO_LDS": "1"}
    assert run(env_exe, env)["now"] == {
        "enc_sorted": "4", "enc_ml": "3", "enc_sorted_ml": "11", "density_fused": "0",
        "density_levels": "16", "shade_bwd_split": "0", "bwd_overlap": "0",
        "bwd_bin_scale": "1e+09", "enc_order": "1:1:3,2,1,0", "enc_simple": "1",
        "enc_simple_h": "2", "enc_simple_rays": "3", "sort_exact": "0", "components_no_lds": "1"}


def test_reload_publishes_a_new_snapshot_and_leaves_the_held_one_alone(env_exe):
    """Started with BIN_SCALE=60, OVERLAP on, ENC_ORDER set; then BIN_SCALE=1e9,
    OVERLAP=0, ENC_ORDER removed, and a reload: the new snapshot reads the new values,
    the reference taken before still reads the old ones (a snapshot is not rewritten in
    place), also after one more reload."""
    start = {"UCSA_BWD_BIN_SCALE": "60", "UCSA_ENC_ORDER": "2:0,1", "UCSA_ENC_SORTED": "1"}
    out = run(env_exe, start, "UCSA_BWD_BIN_SCALE=1e9", "UCSA_BWD_OVERLAP=0", "UCSA_ENC_ORDER",
              "UCSA_DENSITY_LEVELS=8")
    old = {**DEFAULTS, "bwd_bin_scale": "60", "enc_order": "1:2:0,1", "enc_sorted": "1"}
    new = {**DEFAULTS, "bwd_bin_scale": "1e+09", "bwd_overlap": "0", "enc_sorted": "1",
           "density_levels": "8"}
    assert out["now"] == new
    assert out["held"] == old
    assert out["same_object"] == "0"
    assert out["held2"] == old and out["now2"] == new

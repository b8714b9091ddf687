"""CPU: conv_switches_read (csrc/net_conv_switches.h) reads every environment switch of the conv net from one table.  It replaced
the parsing written out in grl_net_create; that parsing is restated below in Python, one function per dialect, each citing the lines
of net_conv.hip at commit 191a583 (the parent of the table) it restates, and a small host program that includes the header is held
to it on every switch and every string of VALUES.  The dialects differ on purpose: tests, bench.py and tools pass these strings.
The header is plain host code: for a sanitizer run, build the program below with -fsanitize=address,undefined and run it directly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "golds-rl-gym_amd", "csrc")

SRC = r"""
#include <stdio.h>
#include <map>
#include <string>
#include "net_conv_switches.h"

static std::map<std::string, std::string> g_env;
static const char *lookup(const char *name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

static void report() {
    grl::ConvSwitches s;
    const char *err = nullptr;
    if (grl::conv_switches_read(lookup, &s, &err)) { printf("refused %s\n", err); return; }
    for (const grl::ConvSwitchRow &r : grl::kConvSwitches)
        if (r.field) printf("%s=%d ", r.name, s.*r.field);
    printf("keep_free_capped=%d keep_free_cap=%llu\n", s.keep_free_capped ? 1 : 0, (unsigned long long)s.keep_free_cap);
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "defaults") {      // a ConvSwitches nobody read into, in report()'s format
        const grl::ConvSwitches s;
        for (const grl::ConvSwitchRow &r : grl::kConvSwitches)
            if (r.field) printf("%s=%d ", r.name, s.*r.field);
        printf("keep_free_capped=%d keep_free_cap=%llu\n", s.keep_free_capped ? 1 : 0, (unsigned long long)s.keep_free_cap);
        return 0;
    }
    if (argc > 1) {      // the table's names, one per line
        for (const grl::ConvSwitchRow &r : grl::kConvSwitches) printf("%s\n", r.name);
        return 0;
    }
    // stdin: cases of `NAME=value` lines (the value is the rest of the line, as it is), each closed by a line with a single dot
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        std::string l(line);
        if (!l.empty() && l.back() == '\n') l.pop_back();
        if (l == ".") { report(); g_env.clear(); continue; }
        const size_t eq = l.find('=');
        if (eq == std::string::npos) return 2;
        g_env[l.substr(0, eq)] = l.substr(eq + 1);
    }
    return 0;
}
"""

UNSET = None
VALUES = (UNSET, "", "off", "OFF", "0", "1", "on", "f32", "lds", "prod", "2", "-1", "3", "127", "128", "255", "256", "512", "1000", "1024",
          "4096", "4097", "8192", "9", "abc", " 4", "4x")


def atoi(s):
    """C's atoi on these strings: white space, a sign, digits; 0 where no number starts"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    return int(m.group(1)) if m else 0


# ---- the dialects of the parent's grl_net_create (net_conv.hip at 191a583).  s is None: the variable is not set
def off_only(s):
    """:1058-1059 GRL_NET_LOSS_SCALE, :1060/:1062 GRL_NET_RANGE_FALLBACK, :1067-1068 GRL_PATCH_SKIP, :1069-1070 GRL_OBS_INDEX,
    :1071-1072 GRL_TRUNK_SKIP, :1077 GRL_NET_ACC1 -- `(e && strcmp(e, "off") == 0) ? 0 : 1`"""
    return 0 if s == "off" else 1


def off_or_0(s):
    """:1082-1083 GRL_PATCH_WGRAD_PAIR, :1084-1085 GRL_PATCH_DGRAD_PAIR, :1086-1087 GRL_SLOT_WGRAD_PAIR, :1088-1089 GRL_SLOTS_XCD --
    default 1; `strcmp(e, "off") != 0 && strcmp(e, "0") != 0`.  :1130-1131 GRL_NET_IDX_SIDE -- `!(e && (!strcmp(e, "off") ||
    !strcmp(e, "0")))`: the same function of the string"""
    return 1 if s is None else int(s != "off" and s != "0")


def keyword(word, default, hit):
    """:1060-1061 GRL_NET_GEMM (f32: 1, else 0), :1074-1075 GRL_NET_EXPAND2 (lds: 0, else 1), :1076 GRL_NET_EXPAND3 (prod: 0, else 1)"""
    return lambda s: hit if s == word else default


def off_or_count(s):
    """:1065-1066 GRL_NET_RANGE_RETURN -- default 4; `strcmp(rr, "off") == 0 ? 0 : std::max(0, atoi(rr))`"""
    return 4 if s is None else 0 if s == "off" else max(0, atoi(s))


def int_unchecked(default):
    """:1045/:1047 GRL_NET_KEEP_LEVEL (default 3), :1079/:1081 GRL_PATCH_WGRAD_XCD (default 1) -- `atoi(e)`"""
    return lambda s: default if s is None else atoi(s)


def int_nonzero(s):
    """:1092/:1096 GRL_PATCH_DGRAD_XCD -- default 1; `atoi(e) != 0`"""
    return 1 if s is None else int(atoi(s) != 0)


def int_floor(s):
    """:1090-1091 GRL_SLOT_WGRAD_CHUNKS -- default 0; `std::max(0, atoi(e))`"""
    return 0 if s is None else max(0, atoi(s))


def int_in_range(default, lo, hi):
    """:1093-1094 GRL_TN_WGS (1024; 256..4096), :1095 GRL_TN_WGS_DENSE (512; 128..4096) -- `if (v >= lo && v <= hi) field = v`.
    :1105-1106 GRL_NET_LANES (1..GRL_MAX_LANES = 8) -- the same, over `(reserved & SINGLE_STREAM) ? 1 : 4`: the header hands back 0
    where the parent kept that flag-dependent default, and grl_net_create puts the default in"""
    return lambda s: default if s is None or not lo <= atoi(s) <= hi else atoi(s)


def int_in_set(s):
    """:1079-1080 GRL_PATCH_SLICE -- default PATCH_SLICE_ROWS = 1024 (net_patch.inc:93); one of six values, else ignored"""
    return atoi(s) if s is not None and atoi(s) in (256, 512, 1024, 2048, 4096, 8192) else 1024


def free_mb(s):
    """:1026-1034 and :1048 GRL_NET_KEEP_FREE_MB -- strtoull(e, &end, 10); refused when `*e < '0' || *e > '9' || *end != 0 ||
    free_mb >= (1ull << 44)`.  -> (capped, bytes), or None: refused"""
    if s is None:
        return 0, 0
    if not re.fullmatch(r"[0-9]+", s) or int(s) >= 1 << 44:      # (a number past 2^64 saturates in strtoull: still >= 2^44)
        return None
    return 1, int(s) << 20


PARENT = {
    "GRL_NET_LOSS_SCALE": off_only, "GRL_NET_RANGE_FALLBACK": off_only, "GRL_PATCH_SKIP": off_only, "GRL_OBS_INDEX": off_only,
    "GRL_TRUNK_SKIP": off_only, "GRL_NET_ACC1": off_only,
    "GRL_PATCH_WGRAD_PAIR": off_or_0, "GRL_PATCH_DGRAD_PAIR": off_or_0, "GRL_SLOT_WGRAD_PAIR": off_or_0, "GRL_SLOTS_XCD": off_or_0,
    "GRL_NET_IDX_SIDE": off_or_0,
    "GRL_NET_GEMM": keyword("f32", 0, 1), "GRL_NET_EXPAND2": keyword("lds", 1, 0), "GRL_NET_EXPAND3": keyword("prod", 1, 0),
    "GRL_NET_RANGE_RETURN": off_or_count,
    "GRL_NET_KEEP_LEVEL": int_unchecked(3), "GRL_PATCH_WGRAD_XCD": int_unchecked(1),
    "GRL_PATCH_DGRAD_XCD": int_nonzero,
    "GRL_SLOT_WGRAD_CHUNKS": int_floor,
    "GRL_TN_WGS": int_in_range(1024, 256, 4096), "GRL_TN_WGS_DENSE": int_in_range(512, 128, 4096), "GRL_NET_LANES": int_in_range(0, 1, 8),
    "GRL_PATCH_SLICE": int_in_set,
}
MB = "GRL_NET_KEEP_FREE_MB"


def expected(env):
    """what the parent's grl_net_create made of this environment: {name: value} with the two fields of the cap, or None: refused"""
    cap = free_mb(env.get(MB))
    if cap is None:
        return None
    out = {name: rule(env.get(name)) for name, rule in PARENT.items()}
    out["keep_free_capped"], out["keep_free_cap"] = cap
    return out


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++ / clang++) to build the check with")
    d = tmp_path_factory.mktemp("conv_switches")
    src, exe = d / "switches.cpp", d / "switches"
    src.write_text(SRC)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def read(envs):
        text = "".join("".join("%s=%s\n" % kv for kv in env.items()) + ".\n" for env in envs)
        lines = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
        assert len(lines) == len(envs)
        return [None if l.startswith("refused ") else {k: int(v) for k, v in (f.split("=") for f in l.split())} for l in lines], lines
    read.names = lambda: subprocess.run([str(exe), "names"], check=True, capture_output=True, text=True).stdout.split()
    read.defaults = lambda: subprocess.run([str(exe), "defaults"], check=True, capture_output=True, text=True).stdout
    return read


def test_every_switch_reads_every_string_as_the_parent_did(reader):
    assert sorted(reader.names()) == sorted(list(PARENT) + [MB])
    envs = [{} if v is UNSET else {name: v} for name in reader.names() for v in VALUES]
    envs.append({name: "off" for name in PARENT})      # all at once: the rows do not lean on each other
    envs.append({name: "512" for name in reader.names()})
    got, _ = reader(envs)
    refused = 0
    for env, g in zip(envs, got):
        want = expected(env)
        assert g == want, (env, g, want)
        refused += want is None
    print("environments compared: %d (%d refused)" % (len(envs), refused))
    assert len(envs) == 24 * len(VALUES) + 2 and refused == 11      # the cap refuses "", off, OFF, on, f32, lds, prod, -1, abc, " 4", 4x
    # a default that no string of VALUES moves would leave its row untested
    for name in PARENT:
        assert len({expected({} if v is UNSET else {name: v})[name] for v in VALUES}) > 1, name


def test_the_declared_defaults_are_what_an_empty_environment_reads_as(reader):
    """ConvSwitches' member initialisers and the table's default column say the same thing, and both say what the parent did"""
    _, lines = reader([{}])
    assert reader.defaults().strip() == lines[0].strip()
    declared = {k: int(v) for k, v in (f.split("=") for f in reader.defaults().split())}
    assert declared == expected({})
    assert declared["GRL_NET_KEEP_LEVEL"] == 3


def test_the_free_memory_cap_refuses_what_the_net_refuses(reader):
    """the strings of test_a_free_memory_cap_that_is_no_number_is_refused (test_gpu_keep_levels.py), and the message it matches"""
    texts = ("", "lots", "12GB", "-1", " 5", "1e3", str(1 << 44))
    got, lines = reader([{MB: t} for t in texts])
    assert got == [None] * len(texts)
    assert set(lines) == {"refused GRL_NET_KEEP_FREE_MB must be a number of MB (decimal digits)"}
    got, _ = reader([{MB: "0"}, {MB: str((1 << 44) - 1)}, {MB: "007"}, {}])
    assert [(g["keep_free_capped"], g["keep_free_cap"]) for g in got] == [(1, 0), (1, ((1 << 44) - 1) << 20), (1, 7 << 20), (0, 0)]


# the conv net's prefixes; a name that ends in "_" is a prefix or a wildcard in prose, not a switch
NAME = re.compile(r"\bGRL_(?:NET_|PATCH_|SLOT_|SLOTS_|TN_|OBS_INDEX|TRUNK_SKIP)[A-Z0-9_]*")
# the create flags of the C ABI (bits of grl_net_config.reserved, include/goldsrl_net.h) share the prefix and are no environment switches
FLAG = re.compile(r"GRL_NET_F_")
# read elsewhere (the header's comment says where) and listed under DESIGN.md's table
ELSEWHERE = {"GRL_NET_EVICT", "GRL_NET_CHUNK"}


def _names(text):
    return {n for n in NAME.findall(text) if not n.endswith("_") and not FLAG.match(n)}


def test_the_table_design_md_and_the_users_name_the_same_switches(reader):
    table = set(reader.names())
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design.split("## 8. Conv net switches", 1)[1].split("\n## ", 1)[0]
    rows = {n for line in section.split("\n") if line.startswith("| `GRL_") for n in _names(line.split("|")[1])}
    assert rows == table, (sorted(rows - table), sorted(table - rows))
    assert ELSEWHERE <= _names(section) - rows      # named under the table, not in it
    used = {}
    files = [os.path.join(ROOT, "bench.py")]
    for sub in ("tests", "tools"):
        for base, _, names in os.walk(os.path.join(ROOT, sub)):
            files += [os.path.join(base, n) for n in names if not n.endswith((".pyc", ".so")) and "__pycache__" not in base]
    for path in files:
        try:
            with open(path) as f:
                text = f.read()
        except UnicodeDecodeError:      # a binary under tools/ubench or tests/golden
            continue
        for n in _names(text):
            used.setdefault(n, []).append(os.path.relpath(path, ROOT))
    assert len(files) > 50 and "GRL_NET_LANES" in used and "GRL_TN_WGS_DENSE" in used
    unknown = {n: where for n, where in used.items() if n not in table | ELSEWHERE}
    assert not unknown, unknown

"""What the CPU tests of the C ABI share: include/gsplat_mi355x.h read once, the library's exported functions listed once, the
"header, mirror and library agree" check of a family of entries, and the check of a refused call."""
import functools
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd._abi")


@functools.lru_cache(maxsize=None)
def header_text(comments=False):
    """The header without its comments (or, for the #define lines, with them)."""
    txt = open(os.path.join(ROOT, "include", "gsplat_mi355x.h")).read()
    return txt if comments else re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@functools.lru_cache(maxsize=None)
def header_functions():
    return sorted(set(re.findall(r"\b(gsplat_[a-z0-9_]+)\s*\(", header_text())))


@functools.lru_cache(maxsize=None)
def header_defines():
    """Every integer #define GSPLAT_* of the header: name -> value."""
    found = re.findall(r"^#define\s+(GSPLAT_[A-Z0-9_]+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\s*$", header_text(comments=True), flags=re.M)
    return {k: int(v, 0) for k, v in found}


@functools.lru_cache(maxsize=None)
def exported_functions():
    """The defined dynamic function symbols of the product library."""
    assert os.path.exists(abi.LIB_PATH), "build the library first: python __graft_entry__.py"
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return frozenset(ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TtWw")


def check_entries(entries, family=None, returns=("int", "int64_t"), stubs_in_namespace=False):
    """entries: name -> argument count.  The header declares each (returning one of `returns`) with that many arguments, _abi.SIGNATURES
    lists it with that many, the library exports it; the ABI version is 12 in all three; no other exported symbol contains the word
    (or one of the words) `family`, in either case -- stubs_in_namespace: but for the C++ names of a unit whose kernels live in a
    namespace named after it (_ZN..., __hip...).  Returns name -> the declared parameter list, as the header spells it."""
    params = {}
    for name, n_args in entries.items():
        m = re.search(rf"\b(?:{'|'.join(returns)})\s+{name}\s*\(([^)]*)\)\s*;", header_text())
        assert m, f"{name} is not declared in include/gsplat_mi355x.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in abi.SIGNATURES and len(abi.SIGNATURES[name][1]) == n_args, name
        assert name in exported_functions(), f"{name} is not exported"
        params[name] = m.group(1)
    assert header_defines()["GSPLAT_ABI_VERSION"] == 12 and abi.ABI_VERSION == 12 and abi.lib().gsplat_abi_version() == 12
    words = (family,) if isinstance(family, str) else tuple(family or ())
    stray = [f for f in exported_functions() if any(w in f.lower() for w in words) and f not in entries
             and not (stubs_in_namespace and f.startswith(("_ZN", "__hip")))]
    assert not stray, f"helpers of the {family} entries exported: {stray}"
    return params


def refused(lib, status, name, word=None, detail=False):
    """The call came back as GSPLAT_ERR_BAD_ARG and gsplat_last_error() names the entry, as "name:" (word: and holds that word;
    detail: and says more than the name)."""
    msg = lib.gsplat_last_error()
    assert status == abi.GSPLAT_ERR_BAD_ARG, (name, word, status)
    assert name.encode() + b":" in msg, (name, msg)
    if word is not None:
        assert word.encode() in msg, (name, word, msg)
    if detail:
        assert len(msg) > len(name) + 2, msg

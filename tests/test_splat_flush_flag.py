"""AMVPT_OPT_GENERIC_FLUSH: the Python constant equals the header's, is a bit of its own, and is a flag bit only
(the ABI version stays)."""
import os
import re

from conftest import REPO


def _header_flags():
    flags = {}
    for name in ("amvpt.h", "amvpt_fixed.h"):
        src = open(os.path.join(REPO, "include", name)).read()
        for m in re.finditer(r"(?:#define\s+)?(AMVPT_OPT_[A-Z_]+)\s*=?\s*(\d+)u", src):
            flags[m.group(1)] = int(m.group(2))
    return flags


def test_generic_flush_flag(amvpt_mod):
    flags = _header_flags()
    assert flags["AMVPT_OPT_GENERIC_FLUSH"] == amvpt_mod.OPT_GENERIC_FLUSH == 2048
    assert len(set(flags.values())) == len(flags)                  # no two options share a bit
    assert all(v & (v - 1) == 0 for v in flags.values())           # each is one bit
    for name, value in flags.items():                              # the Python constants follow the headers
        assert getattr(amvpt_mod, name[len("AMVPT_"):]) == value, name
    assert amvpt_mod.hip_lib().amvpt_abi_version() == 12

"""The stream walk's profile slots (enum HxProf in hmp3_amd/csrc/hx_types.h) for the tools that read a -DHX_PROFILE build's
profile: slots() -> {slot: name}, the member's name in lower case without its HX_PROF_ prefix (HX_PROF_SEEK_ACTUAL -> seek_actual)."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmp3_amd", "csrc", "hx_types.h")


def members(path=HEADER):
    """[(member, value)] of enum HxProf in declaration order"""
    src = open(path).read()
    body = re.search(r"enum\s+HxProf\s*\{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [(m, int(v)) for m, v in re.findall(r"(HX_PROF_\w+)\s*=\s*(\d+)", body)]


def slots(path=HEADER):
    return {v: m[len("HX_PROF_"):].lower() for m, v in members(path)}


def slot(name):
    """the slot of one name (as slots() spells it)"""
    return {n: v for v, n in slots().items()}[name]

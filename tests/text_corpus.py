"""A seeded corpus of small core_<n>.txt texts for the trace-text parsers
(dash_parse_core_file, dash_parse_core_text, the device parser): drawn from a
grammar of valid records, then mutated. Shared by test_text_parse.py,
test_text_sanitize.py and test_gpu_text_ingest.py; built once per process.

Valid records home their addresses on nodes 0..2, so a file without planted
faults is accepted at every N >= 3; planted faults are blank lines, bad
opcodes, "WR 0x 5", NULs before a WR's value, and addresses on nodes >= N.
"""
import ctypes
import functools
import random

import numpy as np

FILES = 3000
SEED = 0x7E87


def _hex(rng, addr):
    """addr as %hhx reads it: 0x/0X/no prefix, either case, sometimes extra leading digits
    (the value is taken mod 256)."""
    s = f"{addr:02x}"
    r = rng.random()
    if r < 0.15:
        s = rng.choice("123456789abcdefABCDEF") + rng.choice("0123456789abcdef") + s
    elif r < 0.25 and addr < 16:
        s = f"{addr:x}"
    if rng.random() < 0.5:
        s = s.upper()
    return rng.choice(["0x", "0x", "0X", ""]) + s


def _dec(rng):
    r = rng.random()
    if r < 0.6:
        s = str(rng.randrange(256))
    elif r < 0.8:
        s = str(rng.randrange(256, 100000))      # taken mod 256
    else:
        s = "".join(rng.choice("0123456789") for _ in range(rng.randrange(6, 12)))  # wraps 2^32
    return rng.choice(["", "", "+", "-"]) + s


def _blank(rng):
    return rng.choice([" ", " ", " ", "\t", "  ", " \t", "   "])


def valid_record(rng, room=18, nodes=3):
    """One valid record's content (no newline) of at most `room` bytes."""
    while True:
        addr = (rng.randrange(nodes) << 4) | rng.randrange(16)
        if rng.random() < 0.5:
            s = "RD" + rng.choice([_blank(rng), _blank(rng), ""]) + _hex(rng, addr)
            if rng.random() < 0.15:
                s += rng.choice([" 7", " junk", "\r", "x", " WR"])
        else:
            s = "WR" + _blank(rng) + _hex(rng, addr) + _blank(rng) + _dec(rng)
            if rng.random() < 0.15:
                s += rng.choice([" x", "\r", ".5", " RD"])
        if len(s) <= room:
            return s


def bad_parse_record(rng):
    return rng.choice(["", "rd 0x12", "XX 0x01 2", "R", "RDWR", "WR 0x 5", "WR 0x12", "WR 0x12 x", "RD", "RD zz",
                       "WR 0x12 -", " RD 0x01", "RD 0x01"[:rng.randrange(1, 3)], "WR 0x12\0 5", "R\0D 0x01"])


def bad_addr_record(rng):
    addr = (rng.randrange(8, 16) << 4) | rng.randrange(16)  # homed past every N <= 8
    if rng.random() < 0.5:
        addr = (rng.randrange(3, 8) << 4) | rng.randrange(16)  # past N = 3; past N = 4 from 0x40
    return rng.choice([f"RD 0x{addr:02X}", f"WR 0x{addr:02x} 9", f"RD {addr:x}"])


def long_line(rng, total):
    """A line of `total` bytes, newline included: full 19-byte chunks, each a valid record
    padded with blanks (trailing bytes are ignored), then the rest."""
    out = ""
    while total - len(out) > 19:
        out += valid_record(rng, 19).ljust(19, rng.choice(" \t"))
    rest = total - len(out) - 1
    if rest >= 7:
        out += valid_record(rng, rest).ljust(rest)
    else:
        out += "Z" * rest  # too short for a record: an empty or junk tail (DASH_EPARSE)
    return out + "\n"


def _line(rng, content):
    return content + rng.choice(["\n", "\n", "\n", "\r\n"] if len(content) < 18 else ["\n"])


def make_file(rng, k):
    kind = k % 8
    n = rng.randrange(0, 61)
    lines = [_line(rng, valid_record(rng)) for _ in range(n)]
    if kind == 1 and n:                         # a planted parse fault
        lines[rng.randrange(n)] = bad_parse_record(rng) + "\n"
    elif kind == 2 and n:                       # a planted address fault
        lines[rng.randrange(n)] = bad_addr_record(rng) + "\n"
    elif kind == 3:                             # 32 accepted records, then bad text past the cap
        lines = [_line(rng, valid_record(rng)) for _ in range(32)]
        lines += [rng.choice([bad_parse_record(rng), bad_addr_record(rng)]) + "\n" for _ in range(rng.randrange(1, 20))]
    elif kind == 4:                             # long lines at the lengths where the split changes
        for _ in range(rng.randrange(1, 4)):
            lines.insert(rng.randrange(len(lines) + 1), long_line(rng, rng.choice([18, 19, 20, 37, 38, 39])))
    elif kind == 5:                             # a 19-byte first chunk, then a valid continuation
        for _ in range(rng.randrange(1, 3)):
            lines.insert(rng.randrange(len(lines) + 1), long_line(rng, rng.choice([27, 30, 38, 46, 57])))
    elif kind == 6 and n:                       # NULs: after an RD's number they change nothing
        i = rng.randrange(n)
        lines[i] = rng.choice(["RD 0x12\0junk\n", "WR 0x12 5\0 9\n", "RD 0x1\0" + "2\n", "RD 0x\n"])
    text = "".join(lines)
    if rng.random() < 0.2 and text.endswith("\n"):
        text = text[:-1]                        # a missing final newline
    return text.encode("latin-1")


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(SEED)
    return tuple(make_file(rng, k) for k in range(FILES))


def parse_file(dash, path, num_procs, max_instr):
    """dash_parse_core_file without raising: (words, rc)."""
    out = np.zeros(max(max_instr, 1), dtype=np.uint16)
    n = ctypes.c_uint32(0)
    rc = dash.lib().dash_parse_core_file(str(path).encode(), num_procs, max_instr, out.ctypes.data, ctypes.byref(n))
    return out[:n.value].copy(), rc


def accepted(dash, num_procs, max_instr):
    """Indices of the corpus files the in-memory parser accepts whole (rc OK), with their words."""
    good = []
    for i, data in enumerate(corpus()):
        words, rc = dash.parse_core_text(data, num_procs, max_instr)
        if rc == dash.OK:
            good.append((i, words))
    return good

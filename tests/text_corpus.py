"""A seeded corpus of small core_<n>.txt texts for the trace-text parsers
(dash_parse_core_file, dash_parse_core_text, the device parser): drawn from a
grammar of valid records, then mutated. Shared by test_text_parse.py,
test_text_sanitize.py and test_gpu_text_ingest.py; built once per process.

A second corpus, scanf_corpus(), and an enumeration of short records, enumeration(), are
seeded separately and leave the first untouched. Their grammar draws what the C library's
sscanf takes and a hand-written scanner may not: signs on the hex number, every isspace
byte as a blank, a 0x without a digit, hex numbers at the saturation edge, the odd corners
of the decimal value. They are judged by tests/sscanf_ref.py (test_text_sscanf.py,
test_gpu_text_sscanf.py).

Valid records home their addresses on nodes 0..2, so a file without planted
faults is accepted at every N >= 3; planted faults are blank lines, bad
opcodes, NULs before a WR's value, and addresses on nodes >= N. bad_parse_record
still draws "WR 0x 5" (the corpus stays byte for byte), which is an accepted
record: the library reads it as address 0, value 5. So bad_parse_record is no
list of rejected records only; the parsers' verdicts, not the generator, say
what a file is.
"""
import ctypes
import functools
import itertools
import random
import re

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


# ---------------------------------------------------------------- the second corpus
# What sscanf("RD %hhx") / sscanf("WR %hhx %hhu") of the C library takes beyond the grammar above.
# Nothing here says what a record parses to: tests/sscanf_ref.py (the library itself) does.

SCANF_FILES = 1500
SCANF_SEED = 0x5CA9F
ENUM_SEED = 0xE9
SPACE = " \t\r\v\f"  # isspace without '\n', which ends a record


def _sp(rng, least=1):
    """A run of isspace bytes: mostly one; least = 0 allows none."""
    return "".join(rng.choice(SPACE) for _ in range(rng.choice([least, 1, 1, 1, 2, 3])))


def _shex(rng, addr):
    """addr as the library's %hhx reads it: a sign ('-' negates, mod 256) or none, 0x/0X or
    none, sometimes digits above the low byte."""
    neg = rng.random() < 0.4
    v = (256 - addr) % 256 if neg else addr
    if rng.random() < 0.3:
        v += 256 * rng.randrange(1, 1 << 12)
    s = f"{v:x}" if rng.random() < 0.5 else f"{v:02X}"
    return ("-" if neg else rng.choice(["+", "+", ""])) + rng.choice(["0x", "0X", "", ""]) + s


def _full(rng, addr):
    """A 19-byte record without newline: RD and 15, 16 or 17 hex digits that stay below the
    saturation edge of a 64-bit long (17 digits: the first is 0)."""
    lo, neg_lo = f"{addr:02x}", f"{(256 - addr) % 256:02x}"
    rnd = lambda n: "".join(rng.choice("0123456789abcdefABCDEF") for _ in range(n))
    return rng.choice([
        "RD0" + rnd(14) + lo, "RD00" + rnd(13) + lo,                                  # 17 digits
        "RD" + rng.choice(SPACE) + rnd(14) + lo, "RD+" + rnd(14) + lo, "RD-" + rnd(14) + neg_lo,
        "RD-" + "f" * 14 + neg_lo,                                                    # 16 digits
        "RD0x" + rnd(13) + lo, "RD" + _sp(rng)[:1] + "-" + rnd(13) + neg_lo, "RD\r\f" + rnd(13) + lo,  # 15
    ])


def scanf_record(rng, nodes=3, node=None):
    """One record's content from the new classes that the library accepts, homed on nodes
    0..nodes-1 (on `node` if given; a digitless 0x reads 0 all the same): at most 18 bytes (a
    newline follows), or exactly 19 (none does)."""
    while True:
        addr = ((rng.randrange(nodes) if node is None else node) << 4) | rng.randrange(16)
        hx = lambda: rng.choice(["0x", "0X", ""]) + f"{addr:02x}"
        dec = lambda: rng.choice(["", "+", "-"]) + str(rng.randrange(300))
        kind = rng.randrange(6)
        if kind == 0:    # a sign on the hex number
            s = "RD" + _sp(rng, 0) + _shex(rng, addr) if rng.random() < 0.5 else \
                "WR" + _sp(rng, 0) + _shex(rng, addr) + _sp(rng) + dec()
        elif kind == 1:  # every isspace byte as a blank: after the opcode, before the value, trailing
            s = "RD" + _sp(rng) + hx() + _sp(rng, 0) if rng.random() < 0.5 else \
                "WR" + _sp(rng) + hx() + _sp(rng) + dec() + _sp(rng, 0)
        elif kind == 2:  # 0x / 0X without a digit: address 0
            pre = _sp(rng, 0) + rng.choice(["", "", "+", "-"]) + rng.choice(["0x", "0X"])
            s = "RD" + pre + rng.choice([" 5", "\r", "-", "+1", "g", "", "\0junk", " \t7", "x1"]) if rng.random() < 0.5 else \
                "WR" + pre + rng.choice([" 5", "\r7", "-5", "+5", " -5", "\f\v9", "\t0x5"])
        elif kind == 3:  # 8 and 9 hex digits
            n = rng.choice([8, 9])
            d = f"{rng.randrange(16 ** (n - 3), 16 ** (n - 2)):x}{addr:02x}"
            s = "RD " + d if rng.random() < 0.5 else "WR " + rng.choice(["", "0x"]) + d + " " + dec()
        elif kind == 4:  # the decimal side
            s = "WR " + hx() + rng.choice([" 0x5", " -0", " +0", "\r0x", " 00", " -256", "-1", "+7", " 0X9"])
        else:
            s = _full(rng, addr)
        if len(s) <= 19:
            return s


def scanf_bad_parse(rng):
    """Records of the new classes in which the library assigns fewer fields than the format has."""
    return rng.choice(["RD -", "RD +g", "WR 1 \r", "WR -", "RD - 1", "WR 1 - 5", "WR 1 +", "WR 1 -", "WR 0xg 5",
                       "WR 0x", "WR 0X\r", "WR 0x\0 5", "RD\r", "WR\f1\v", "RD +-1", "RD x1", "WR 1 x5", "WR+ 1 5",
                       "RD\v\f", "WR 0x+", "WR 1\0 5"])


def scanf_bad_addr(rng):
    """Records the library parses to an address past every N <= 8 (or past N = 3 / 4): negative
    numbers, the low byte of long ones, and 17 significant hex digits, which saturate to 0xFF."""
    return rng.choice(["RD -1", "RD -0x10", "WR +ff 1", "RD\r0x80", "WR\v-0X01\f7", "RD12345678901234567",
                       "RDffffffffffffffff1", "RD10000000000000012", "RD -0xd0", "WR\v-c0 1", "RD +0x1234567a0",
                       "RD-ffffffffffffff60"])


def _join(rng, contents):
    """Records to text: a 19-byte record is followed by no newline (one would be an empty record)."""
    return "".join(c if len(c) == 19 else c + rng.choice(["\n", "\n", "\n", "\r\n"] if len(c) < 18 else ["\n"])
                   for c in contents)


def make_scanf_file(rng, k):
    kind = k % 6
    n = rng.randrange(0, 41)
    recs = [scanf_record(rng) for _ in range(n)]
    if kind == 1 and n:                         # a parse fault from the new classes
        recs[rng.randrange(n)] = scanf_bad_parse(rng)
    elif kind == 2 and n:                       # an address fault from the new classes
        recs[rng.randrange(n)] = scanf_bad_addr(rng)
    elif kind == 3:                             # 32 accepted records, then bad text past the cap
        recs = [scanf_record(rng) for _ in range(32)]
        recs += [rng.choice([scanf_bad_parse, scanf_bad_addr, bad_parse_record])(rng) for _ in range(rng.randrange(1, 9))]
    elif kind == 4 and n:                       # the present fault classes
        recs[rng.randrange(n)] = rng.choice([bad_parse_record, bad_addr_record])(rng)
    elif kind == 5 and n:                       # the present valid records among the new ones
        for _ in range(rng.randrange(1, 6)):
            recs[rng.randrange(n)] = valid_record(rng)
    text = _join(rng, recs)
    if rng.random() < 0.2 and text.endswith("\n"):
        text = text[:-1]
    return text.encode("latin-1")


@functools.lru_cache(maxsize=None)
def scanf_corpus():
    rng = random.Random(SCANF_SEED)
    return tuple(make_scanf_file(rng, k) for k in range(SCANF_FILES))


_H = rb"[0-9a-fA-F]"
# The four deviation classes of DESIGN.md §5.3 as patterns over one record (re.match): each is
# a record the library accepts and a scanner that takes ' ' and '\t', no sign, a 0x only before
# a digit, and the number mod 256 does not, or reads differently.
DEVIATIONS = {
    "sign": rb"(RD|WR)\s*[+-]",
    "blank": rb"(RD|WR)[ \t]*[\r\v\f]|WR\s*[+-]?\w+[ \t]*[\r\v\f]\s*[+-]?\d",
    "digitless 0x": rb"WR\s*[+-]?0[xX](?!" + _H + rb")",
    "saturation": rb"RD0*[1-9a-fA-F]" + _H + rb"{16}",
}
# name -> (pattern, does the library accept such a record?): what the second corpus must hold
CLASSES = {
    **{name: (pat, True) for name, pat in DEVIATIONS.items()},
    "sign with 0x": (rb"(RD|WR)\s*[+-]0[xX]" + _H, True),
    "sign without 0x": (rb"(RD|WR)\s*[+-](?!0[xX])" + _H, True),
    "blank run": (rb"(RD|WR)[ \t\r\v\f]*[\r\v\f][ \t\r\v\f]+\S", True),
    "trailing blank": (rb"WR\s*\S+\s+[+-]?\d+[\r\v\f]", True),
    # a 0x / 0X without a hex digit, by what follows it, in RD and in WR: an RD has its number (the
    # 0) whatever follows; a WR needs a value after it
    **{f"0x then {what}, {op.decode()}": (op + rb"\s*[+-]?0[xX]" + follower, accepted)
       for what, follower, wr_accepted in (("blank", rb"[ \t\r\v\f]", True), ("sign", rb"[+-]", True),
                                           ("blank and digit", rb"[ \t\r\v\f]+\d", True), ("g", rb"g", False),
                                           ("the end", rb"\n?$", False), ("NUL", rb"\0", False))
       for op, accepted in ((b"RD", True), (b"WR", wr_accepted))},
    # every isspace byte in every position: after the opcode, before the value, trailing
    **{f"{name} {where}": (pat.replace(b"B", re.escape(byte)), True)
       for name, byte in (("space", b" "), ("tab", b"\t"), ("CR", b"\r"), ("VT", b"\v"), ("FF", b"\f"))
       for where, pat in (("after the opcode", rb"(RD|WR)[ \t\r\v\f]*B[ \t\r\v\f]*[+-]?[0-9a-f]"),
                          ("before the value", rb"WR[ \t\r\v\f]*[+-]?[0-9a-fxX]+[ \t\r\v\f]*B[ \t\r\v\f]*[+-]?\d"),
                          ("trailing, RD", rb"RD[ \t\r\v\f]*[+-]?[0-9a-fxX]+[ \t\r\v\f]*B"),
                          ("trailing, WR", rb"WR[ \t\r\v\f]*[+-]?[0-9a-fxX]+[ \t\r\v\f]*[+-]?\d+[ \t\r\v\f]*B"))},
    **{f"{n} hex digits": (rb"(RD|WR)\s*[+-]?(0[xX])?" + _H + (b"{%d}(?!" % n) + _H + rb")", True) for n in (8, 9, 15, 16, 17)},
    "value 0x5": (rb"WR\s*\S+\s+0[xX]\d", True),
    "value -0": (rb"WR\s*\S+\s+-0(?!\d)", True),
    "value a lone sign": (rb"WR\s*\S+\s+[+-]\s*$", False),
    "value - 5": (rb"WR\s*\S+\s+[+-]\s+\d", False),
    "sign without number": (rb"(RD|WR)\s*[+-](?![0-9a-fA-F])", False),
    "blank without number": (rb"(RD|WR)\s*[\r\v\f]\s*$", False),
    "present faults": (rb"$|rd|XX|R$|RDWR|RD\n?$|RD zz| RD|R\0", False),
}


def scanf_accepted(twin, num_procs, max_instr):
    """Indices of the second corpus's files the twin accepts whole (rc OK), with their words."""
    good = []
    for i, data in enumerate(scanf_corpus()):
        words, rc = twin.parse_core_text(data, num_procs, max_instr)
        if rc == twin.OK:
            good.append((i, words))
    return good


ALPHABET = b" \t\r\f+-01agxX\n"


@functools.lru_cache(maxsize=None)
def enumeration():
    """Short records around the conversions' decisions, each distinct: every RD / WR followed by
    0 to 4 bytes of ALPHABET, then 20,000 seeded draws of 5 to 17 bytes from ALPHABET + 9 f F."""
    recs = {op + bytes(t): None for op in (b"RD", b"WR") for n in range(5) for t in itertools.product(ALPHABET, repeat=n)}
    exhaustive = len(recs)
    rng = random.Random(ENUM_SEED)
    wide = ALPHABET + b"9fF"
    for _ in range(20000):
        n = rng.randrange(5, 18)
        recs.setdefault(rng.choice([b"RD", b"WR"]) + bytes(rng.choice(wide) for _ in range(n)))
    return tuple(recs), exhaustive

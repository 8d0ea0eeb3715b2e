"""The yardstick of the trace-text parsers (test infrastructure): the reference's ingest
(initializeProcessor, ref :831-847) with the C library's own sscanf doing the fields.

parse_core_text(data, num_procs, max_instr) has the signature and the verdicts of
dash.parse_core_text and shares no code with dash_parse_core_file, dash_parse_core_text or
the device parser:

  Record   fgets(line, 20): up to 19 bytes, through the first '\\n'; the content ends at the
           first NUL (a C string). Reading stops once max_instr records are accepted or the
           bytes run out.
  Fields   sscanf(line, "RD %hhx", &a) / sscanf(line, "WR %hhx %hhu", &a, &v) of the C library
           this process has loaded (through ctypes), the formats as the reference spells them.
  Verdict  A record that starts "RD" with return value 1, or "WR" with return value 2, is
           accepted with the bytes sscanf assigned (an RD's value is 0, ref :839). Any other
           record is EPARSE: the reference would execute fields nobody assigned. The address
           check (addr >> 4 >= num_procs: EADDR) comes after a successful parse.

The yardstick is the library's behaviour, also where the C standard would allow another (a
"0x" without a hex digit is consumed and reads as 0 in glibc).
"""
import ctypes
import functools

import numpy as np

OK, EPARSE, EADDR = 0, -3, -4  # DASH_OK, DASH_EPARSE, DASH_EADDR (include/dash.h)
RECORD = 19                    # fgets(line, 20)

_libc = ctypes.CDLL(None)
# what a C99 compiler links for sscanf in glibc; the plain name elsewhere
_sscanf = getattr(_libc, "__isoc99_sscanf", None) or _libc.sscanf
_sscanf.restype = ctypes.c_int


@functools.lru_cache(maxsize=1 << 18)
def scan_record(rec: bytes):
    """One record (the bytes fgets returned) -> (is_wr, addr, val), or None when the reference
    would run an instruction with unassigned fields."""
    line = ctypes.create_string_buffer(rec, len(rec) + 1)  # NUL-terminated, like fgets' buffer
    a, v = ctypes.c_ubyte(0xA5), ctypes.c_ubyte(0x5A)
    if rec[:2] == b"RD":
        got = _sscanf(line, ctypes.c_char_p(b"RD %hhx"), ctypes.byref(a))
        return (False, a.value, 0) if got == 1 else None
    if rec[:2] == b"WR":
        got = _sscanf(line, ctypes.c_char_p(b"WR %hhx %hhu"), ctypes.byref(a), ctypes.byref(v))
        return (True, a.value, v.value) if got == 2 else None
    return None


def records(data: bytes):
    """fgets(line, 20) over the bytes: successive records, each with its extent."""
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos, pos + RECORD)
        end = nl + 1 if nl >= 0 else min(pos + RECORD, len(data))
        yield data[pos:end]
        pos = end


def parse_core_text(data, num_procs, max_instr):
    data = bytes(data)
    words, rc = [], OK
    if max_instr > 0:
        for rec in records(data):
            got = scan_record(rec)
            if got is None:
                rc = EPARSE
                break
            wr, addr, val = got
            if (addr >> 4) >= num_procs:
                rc = EADDR
                break
            words.append(((0x8000 if wr else 0) | (addr << 8) | val) & 0xFFFF)
            if len(words) == max_instr:
                break
    return np.array(words, dtype=np.uint16), rc


def accepts(rec: bytes) -> bool:
    """Does the reference run a well-defined instruction for this one record?"""
    return scan_record(rec) is not None

"""Python view of libdash (the C-ABI in include/dash.h) -- the host-side mirror
of the reference's interface for the hot path.

The reference (assignment.c) exposes: the CLI `./cache_simulator <dir>`
(:126-131), initializeProcessor (:806-851), the per-thread event loop
(:149-738) and printProcessorState (:853-905). This module maps them onto
libdash:

    parse_core_file(path)          -> initializeProcessor's parse (:822-850)
    parse_core_text(bytes)         -> the same parse on bytes in memory
    Engine(...).load_dir(dir)      -> initializeProcessor per node (:152)
    Engine.load_text(blobs)        -> the same parse on the GPU, many systems per call
    Engine.load_dirs(dirs, device) -> bulk directory ingest, parsed on the host or the GPU
    Engine.run()                   -> the OpenMP parallel region (:149-738)
    Engine.explore(src, s0, k)     -> the outcomes k seeded legal schedules of one system reach
    Engine.explore_micro(src, s0, k, weights) -> the same over seeded micro-step schedules
    Engine.explore_sources(g, s0, k) -> the outcomes of g trace sets at once, merged and classified on
                                      the GPU (counts, witnesses, coherence records; explore_assign
                                      states which system runs which source and seed)
    Engine.explore_delays(g, R, E, D) -> the same over every schedule within D delays of lockstep
                                      (delay_count, delay_word and delay_schedule state the space;
                                      set_system_delays runs chosen delay words)
    Engine.shrink_many(jobs)       -> many (system, seed, goal) jobs shrunk side by side in one call, each
                                      to where Engine.shrink takes it alone (shrink_assign states how
                                      a sub-pass's systems are dealt out)
    Engine.shrink(src, coh_all)    -> one system cut down on the GPU to a 1-minimal trace set that still
                                      ends with those coherence bits (shrink_candidate states the
                                      candidates of a round; write_dir writes the result as core_<n>.txt)
    Engine.read_state(sys)         -> the nodes' processorNode state
    Engine.compute_metrics()       -> per-node miss / invalidation / wait metrics, reduced on the GPU
                                      from the event log (read_metrics returns the records)
    Engine.compute_addr_metrics()  -> the same log by address: traffic, sharers and a sharing class per
                                      cache line (read_addr_metrics returns the records; addr_class and
                                      addr_metrics_from_events are the same rules on the host)
    Engine.check_coherence()       -> the coherence invariants of every final state, checked on the GPU
                                      (read_coherence returns the records; check_outcomes classifies
                                      an explore's outcomes; check_states is the same on the host)
    Engine.write_states(first, l)  -> testing only: hand-built states in place of the run's, for
                                      check_coherence (dash_test_write_states)
    dump_node(state, node)         -> printProcessorState bytes (:868-902)
    simulate_dir(dir, out_dir)     -> main() end to end

There is no CPU fallback: if libdash.so is missing or no HIP device is
present the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import subprocess

import numpy as np

PKG = pathlib.Path(__file__).resolve().parent
# DASH_LIB: an alternative build of the same library (kernel variant experiments, tools/)
LIB_PATH = pathlib.Path(os.environ["DASH_LIB"]) if os.environ.get("DASH_LIB") else PKG / "libdash.so"

MEM_SIZE = 16
MAX_PROCS = 8
MAX_CACHE = 16
NUM_TXN = 13
TXN_NAMES = ("READ_REQUEST", "WRITE_REQUEST", "REPLY_RD", "REPLY_WR", "REPLY_ID", "INV",
             "UPGRADE", "WRITEBACK_INV", "WRITEBACK_INT", "FLUSH", "FLUSH_INVACK",
             "EVICT_SHARED", "EVICT_MODIFIED")

OK, EINVAL, EIO, EPARSE, EADDR, EDEVICE, ENOMEM, ESTATE, ETRUNC = 0, -1, -2, -3, -4, -5, -6, -7, -8
EV_MSG, EV_INSTR = 0, 1
ERR_OVERFLOW, ERR_OOB, ERR_CTZ0, ERR_DEADLOCK, ERR_ROUNDCAP, ERR_STUCK = 1, 2, 4, 8, 16, 32
ERR_SCHEDULE = 64  # a micro-step schedule stepped a node with held sends (dash.h)
KEEP_STATE = 1
TIER_FROM_32, TIER_FROM_256 = 2, 4
TEST_SHORT_ARB = 8  # testing only (dash.h)
TEST_ONE_GROUP = 16  # testing only (dash.h)
TEST_INSERT_PER_LANE, TEST_INSERT_GROUPS = 32, 64  # testing and measurement only (dash.h)
NUM_TIERS = 3
GEN_UNIFORM, GEN_CONTENTION, GEN_LOCALITY = 0, 1, 2

# every symbol include/dash.h declares
EXPORTS = ("dash_create", "dash_destroy", "dash_last_error", "dash_load_traces", "dash_generate",
           "dash_run", "dash_read_state", "dash_read_results", "dash_read_hist", "dash_stream",
           "dash_parse_core_file", "dash_resolve_dir", "dash_load_dir", "dash_init_node_state",
           "dash_dump_node", "dash_dump_file", "dash_digest_node", "dash_simulate_dir",
           "dash_read_events", "dash_format_event", "dash_load_dirs", "dash_dump_system",
           "dash_write_digests", "dash_run_host_batched", "dash_set_schedule", "dash_probe_box",
           "dash_set_micro_schedule", "dash_parse_core_text", "dash_read_dirs_text", "dash_load_text",
           "dash_load_dirs_device", "dash_read_traces", "dash_ingest_info", "dash_set_system_seeds",
           "dash_broadcast_system", "dash_seed_schedule", "dash_explore", "dash_micro_pick",
           "dash_set_micro_seeds", "dash_read_micro_acts", "dash_explore_micro", "dash_compute_metrics",
           "dash_read_metrics", "dash_check_states", "dash_check_coherence", "dash_read_coherence",
           "dash_check_outcomes", "dash_explore_sources", "dash_explore_assign", "dash_shrink",
           "dash_shrink_candidate", "dash_write_dir", "dash_test_write_states", "dash_shrink_many",
           "dash_shrink_assign", "dash_compute_addr_metrics", "dash_read_addr_metrics", "dash_addr_class",
           "dash_addr_metrics_from_events", "dash_set_system_delays", "dash_delay_schedule", "dash_delay_count",
           "dash_delay_word", "dash_explore_delays")
DELAY_EMPTY, DELAY_LOCKSTEP = 0xFFFF, 0xFFFFFFFFFFFFFFFF  # DASH_DELAY_EMPTY, DASH_DELAY_LOCKSTEP
TEXT_TILE = 4096  # DASH_TEXT_TILE: bytes per tile of the device text parser
SIT_OUT = 0xFF
MICRO_STEP, MICRO_SEND = 0, 1  # dash_set_micro_schedule actions
MICRO_UNIFORM = 0x0101010101010101  # DASH_MICRO_UNIFORM: every node weight 1


class DashError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed with code {code}")
        self.code = code


class Cfg(ctypes.Structure):
    _fields_ = [("num_procs", ctypes.c_uint32), ("cache_size", ctypes.c_uint32),
                ("max_instr", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("num_systems", ctypes.c_uint64), ("max_rounds", ctypes.c_uint64),
                ("device", ctypes.c_int32), ("trace_events", ctypes.c_uint32),
                ("schedule_seed", ctypes.c_uint64)]


class Event(ctypes.Structure):
    _fields_ = [("round", ctypes.c_uint32), ("node", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("word", ctypes.c_uint32)]


class NodeState(ctypes.Structure):
    _fields_ = [("memory", ctypes.c_uint8 * MEM_SIZE), ("dir_bitvector", ctypes.c_uint8 * MEM_SIZE),
                ("dir_state", ctypes.c_uint8 * MEM_SIZE), ("cache_addr", ctypes.c_uint8 * MAX_CACHE),
                ("cache_value", ctypes.c_uint8 * MAX_CACHE),
                ("cache_state", ctypes.c_uint8 * MAX_CACHE)]


class Stats(ctypes.Structure):
    _fields_ = [("hist", ctypes.c_uint64 * NUM_TXN), ("instructions", ctypes.c_uint64),
                ("rounds_total", ctypes.c_uint64), ("rounds_max", ctypes.c_uint64),
                ("systems", ctypes.c_uint64), ("err_systems", ctypes.c_uint64),
                ("err_bits", ctypes.c_uint64), ("dropped", ctypes.c_uint64),
                ("max_depth", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("tier_systems", ctypes.c_uint64 * NUM_TIERS), ("wave_rounds", ctypes.c_uint64)]

    def as_dict(self):
        return {"hist": [int(x) for x in self.hist], "instructions": int(self.instructions),
                "rounds_total": int(self.rounds_total), "rounds_max": int(self.rounds_max),
                "systems": int(self.systems), "err_systems": int(self.err_systems),
                "err_bits": int(self.err_bits), "dropped": int(self.dropped),
                "max_depth": int(self.max_depth), "kernel_ms": float(self.kernel_ms),
                "tier_systems": [int(x) for x in self.tier_systems],
                "wave_rounds": int(self.wave_rounds)}


class BoxProbe(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("arch", ctypes.c_char * 32), ("compute_units", ctypes.c_int32),
                ("clock_khz", ctypes.c_int32), ("mem_clock_khz", ctypes.c_int32), ("pci_domain", ctypes.c_int32),
                ("pci_bus", ctypes.c_int32), ("pci_device", ctypes.c_int32), ("total_mem", ctypes.c_uint64),
                ("probe_ms", ctypes.c_double), ("probe_valu_per_s", ctypes.c_double),
                ("probe_sclk_mhz", ctypes.c_double), ("probe_sclk_min_mhz", ctypes.c_double),
                ("probe_sclk_max_mhz", ctypes.c_double)]


class IngestReport(ctypes.Structure):
    _fields_ = [("rc", ctypes.c_int32), ("record", ctypes.c_uint32), ("file", ctypes.c_uint64),
                ("text_bytes", ctypes.c_uint64), ("read_ms", ctypes.c_double), ("copy_ms", ctypes.c_double),
                ("parse_ms", ctypes.c_double)]


class Outcome(ctypes.Structure):
    _fields_ = [("digest", ctypes.c_uint64), ("count", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("rounds", ctypes.c_uint32), ("errors", ctypes.c_uint32)]


# dash_node_metrics / dash_metrics_totals (include/dash.h states what each field counts)
METRIC_FIELDS = ("reads", "writes", "read_misses", "write_misses", "upgrades", "msgs", "home_requests",
                 "invalidations", "interventions", "evict_shared", "evict_modified", "waits", "wait_rounds",
                 "wait_max", "deliveries", "idle_rounds")
METRICS_DTYPE = np.dtype([(f, np.uint32) for f in METRIC_FIELDS])


class NodeMetrics(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in METRIC_FIELDS]


class MetricsTotals(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in METRIC_FIELDS + ("systems", "truncated_systems")]


# dash_addr_metrics / dash_addr_totals (include/dash.h states what each field counts)
ADDR_METRIC_FIELDS = ("reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations", "interventions",
                      "flushes", "evict_shared", "evict_modified", "msgs", "nodes")
ADDR_METRICS_DTYPE = np.dtype([(f, np.uint32) for f in ADDR_METRIC_FIELDS])
assert ADDR_METRICS_DTYPE.itemsize == 48
ADDR_UNTOUCHED, ADDR_PRIVATE, ADDR_READ_SHARED, ADDR_ONE_WRITER, ADDR_MULTI_WRITER = range(5)  # DASH_ADDR_*
ADDR_CLASS_NAMES = ("untouched", "private", "read_shared", "one_writer", "multi_writer")


class AddrMetrics(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ADDR_METRIC_FIELDS]


class AddrTotals(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ADDR_METRIC_FIELDS[:11] + ("msgs_max", "foreign_events")] + \
               [(f, ctypes.c_uint64 * 5) for f in ("class_addrs", "class_misses", "class_invalidations")] + \
               [(f, ctypes.c_uint64) for f in ("systems", "truncated_systems")]


# DASH_COH_*: the invariants an address can break (include/dash.h states each)
COH_SWMR, COH_DIR_U_HELD, COH_DIR_EM, COH_DIR_S = 1, 2, 4, 8
COH_LOST_SHARER, COH_STALE_SHARER, COH_STALE_VALUE, COH_VALUE_SPLIT = 16, 32, 64, 128
COH_NAMES = ("SWMR", "DIR_U_HELD", "DIR_EM", "DIR_S", "LOST_SHARER", "STALE_SHARER", "STALE_VALUE", "VALUE_SPLIT")
COHERENCE_FIELDS = ("bits", "addrs", "first_addr", "first_bits")
COHERENCE_DTYPE = np.dtype([(f, np.uint32) for f in COHERENCE_FIELDS])


class Coherence(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in COHERENCE_FIELDS]


class CoherenceTotals(ctypes.Structure):
    _fields_ = [("systems", ctypes.c_uint64), ("violating_systems", ctypes.c_uint64),
                ("violating_clean_systems", ctypes.c_uint64), ("addrs", ctypes.c_uint64),
                ("bit_systems", ctypes.c_uint64 * 8), ("bit_addrs", ctypes.c_uint64 * 8)]


# dash_outcome_ex / dash_source_summary / dash_explore_totals (dash_explore_sources): an outcome with
# its coherence record (the COHERENCE_FIELDS, flat) and its source
OUTCOME_EX_DTYPE = np.dtype([("digest", np.uint64), ("count", np.uint64), ("seed", np.uint64), ("rounds", np.uint32),
                             ("errors", np.uint32)] + [(f, np.uint32) for f in COHERENCE_FIELDS] +
                            [("source", np.uint32), ("_reserved", np.uint32)])
SOURCE_SUMMARY_DTYPE = np.dtype([("schedules", np.uint64), ("incoherent_schedules", np.uint64),
                                 ("top_count", np.uint64), ("outcomes", np.uint32),
                                 ("incoherent_outcomes", np.uint32), ("coh_bits", np.uint32), ("err_bits", np.uint32)])
assert OUTCOME_EX_DTYPE.itemsize == 56 and SOURCE_SUMMARY_DTYPE.itemsize == 40


class ExploreTotals(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("schedules", "outcomes", "unplaced", "passes", "table_slots",
                                               "incoherent_outcomes", "incoherent_schedules",
                                               "incoherent_clean_schedules")] + \
               [("bit_schedules", ctypes.c_uint64 * 8), ("sim_ms", ctypes.c_double), ("merge_ms", ctypes.c_double),
                ("insert_ms", ctypes.c_double)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["bit_schedules"] = [int(x) for x in self.bit_schedules]
        return d


# dash_delay_space (dash_delay_count, dash_delay_word, dash_explore_delays)
class DelaySpace(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("starts", "lens", "max_delays", "_reserved")]


# dash_shrink_goal / dash_shrink_step / dash_shrink_report (dash_shrink)
class ShrinkGoal(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("coh_all", "err_all", "err_none", "_reserved")]


SHRINK_STEP_DTYPE = np.dtype([(f, np.uint32) for f in ("node", "start", "count", "candidates")])


class ShrinkReport(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("rounds", "passes", "variants", "instr_before", "instr_after")] + \
               [(f, ctypes.c_double) for f in ("sim_ms", "gen_ms", "select_ms")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# dash_shrink_job / dash_shrink_result / dash_shrink_many_report (dash_shrink_many)
SHRINK_MAX_JOBS = 65536
SHRINK_MINIMAL, SHRINK_UNMET = 0, 1
SHRINK_JOB_DTYPE = np.dtype([("src", np.uint64), ("seed", np.uint64), ("coh_all", np.uint32), ("err_all", np.uint32),
                             ("err_none", np.uint32), ("_reserved", np.uint32)])
SHRINK_RESULT_DTYPE = np.dtype([("status", np.uint32), ("rounds", np.uint32), ("instr_before", np.uint32),
                                ("instr_after", np.uint32), ("variants", np.uint64), ("src_coh_bits", np.uint32),
                                ("src_errors", np.uint32)])
assert SHRINK_JOB_DTYPE.itemsize == 32 and SHRINK_RESULT_DTYPE.itemsize == 32


class ShrinkManyReport(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("jobs", "minimal", "unmet", "rounds", "passes", "variants",
                                               "instr_before", "instr_after")] + \
               [(f, ctypes.c_double) for f in ("sim_ms", "gen_ms", "select_ms")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class Gen(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("sys_base", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("locality", ctypes.c_uint32), ("len", ctypes.c_uint32), ("_reserved", ctypes.c_uint32)]


_lib = None


def build():
    """Compile libdash.so + cache_simulator for gfx950 (in-tree)."""
    subprocess.run(["make", "-s", "-C", str(PKG), f"-j{min(8, os.cpu_count() or 1)}"], check=True)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: run build() first (no CPU fallback exists)")
    L = ctypes.CDLL(str(LIB_PATH))
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    sig = {
        "dash_create": (i32, [ctypes.POINTER(Cfg), ctypes.POINTER(vp)]),
        "dash_destroy": (None, [vp]),
        "dash_last_error": (ctypes.c_char_p, [vp]),
        "dash_load_traces": (i32, [vp, vp, u64, vp, u64]),
        "dash_generate": (i32, [vp, ctypes.POINTER(Gen)]),
        "dash_set_schedule": (i32, [vp, vp, u32]),
        "dash_set_micro_schedule": (i32, [vp, vp, u32]),
        "dash_probe_box": (i32, [i32, ctypes.POINTER(BoxProbe)]),
        "dash_run": (i32, [vp, ctypes.POINTER(Stats)]),
        "dash_read_state": (i32, [vp, u64, ctypes.POINTER(NodeState)]),
        "dash_test_write_states": (i32, [vp, u64, u64, ctypes.POINTER(NodeState)]),
        "dash_read_results": (i32, [vp, u64, u64, vp, vp, vp]),
        "dash_read_hist": (i32, [vp, u64, vp]),
        "dash_stream": (vp, [vp]),
        "dash_parse_core_file": (i32, [ctypes.c_char_p, u32, u32, vp, ctypes.POINTER(u32)]),
        "dash_resolve_dir": (i32, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]),
        "dash_load_dir": (i32, [vp, ctypes.c_char_p, u64]),
        "dash_init_node_state": (None, [ctypes.POINTER(NodeState), u32, u32]),
        "dash_dump_node": (i32, [ctypes.POINTER(NodeState), u32, u32, ctypes.c_char_p, ctypes.c_size_t]),
        "dash_dump_file": (i32, [ctypes.POINTER(NodeState), u32, u32, ctypes.c_char_p]),
        "dash_digest_node": (u64, [ctypes.POINTER(NodeState), u32, u32]),
        "dash_simulate_dir": (i32, [ctypes.c_char_p, u32, u32, u32, ctypes.c_char_p, i32,
                                    ctypes.POINTER(Stats)]),
        "dash_read_events": (i32, [vp, u64, vp, u32, ctypes.POINTER(u32)]),
        "dash_load_dirs": (i32, [vp, ctypes.POINTER(ctypes.c_char_p), u64]),
        "dash_dump_system": (i32, [vp, u64, ctypes.c_char_p]),
        "dash_write_digests": (i32, [vp, ctypes.c_char_p]),
        "dash_format_event": (i32, [ctypes.POINTER(Event), ctypes.c_char_p, ctypes.c_size_t]),
        "dash_run_host_batched": (i32, [ctypes.POINTER(Cfg), vp, u64, vp, u64, u32, ctypes.POINTER(Stats),
                                        vp, vp, vp]),
        "dash_parse_core_text": (i32, [ctypes.c_char_p, ctypes.c_size_t, u32, u32, vp, ctypes.POINTER(u32)]),
        "dash_read_dirs_text": (i32, [ctypes.POINTER(ctypes.c_char_p), u64, u32, u32, vp, u64, vp, vp,
                                      ctypes.POINTER(u64)]),
        "dash_load_text": (i32, [vp, vp, vp, vp, u64]),
        "dash_load_dirs_device": (i32, [vp, ctypes.POINTER(ctypes.c_char_p), u64]),
        "dash_read_traces": (i32, [vp, vp, u64, vp]),
        "dash_ingest_info": (i32, [vp, ctypes.POINTER(IngestReport)]),
        "dash_set_system_seeds": (i32, [vp, vp, u64]),
        "dash_broadcast_system": (i32, [vp, u64]),
        "dash_seed_schedule": (i32, [u64, u32, u32, vp]),
        "dash_explore": (i32, [vp, u64, u64, u64, vp, u32, ctypes.POINTER(u32)]),
        "dash_micro_pick": (i32, [u64, u32, u32, u64, u32]),
        "dash_set_micro_seeds": (i32, [vp, vp, vp, u64]),
        "dash_read_micro_acts": (i32, [vp, u64, vp, u32, ctypes.POINTER(u32)]),
        "dash_explore_micro": (i32, [vp, u64, u64, u64, u64, vp, u32, ctypes.POINTER(u32)]),
        "dash_compute_metrics": (i32, [vp, ctypes.POINTER(MetricsTotals)]),
        "dash_read_metrics": (i32, [vp, u64, u64, vp, vp]),
        "dash_check_states": (i32, [ctypes.POINTER(NodeState), u32, u32, ctypes.POINTER(Coherence), vp]),
        "dash_check_coherence": (i32, [vp, ctypes.POINTER(CoherenceTotals)]),
        "dash_read_coherence": (i32, [vp, u64, u64, vp]),
        "dash_check_outcomes": (i32, [vp, u64, vp, u32, ctypes.POINTER(u64), vp]),
        "dash_explore_sources": (i32, [vp, u64, u64, u64, ctypes.POINTER(u64), u64, vp, u64, ctypes.POINTER(u64), vp,
                                       ctypes.POINTER(ExploreTotals)]),
        "dash_explore_assign": (i32, [u64, u64, u64, u64, u64, u64, ctypes.POINTER(u32), ctypes.POINTER(u64),
                                      ctypes.POINTER(i32)]),
        "dash_shrink": (i32, [vp, u64, u64, ctypes.POINTER(ShrinkGoal), vp, u64, vp, vp, u32, ctypes.POINTER(u32),
                              ctypes.POINTER(ShrinkReport)]),
        "dash_shrink_candidate": (i32, [vp, u32, u64, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "dash_write_dir": (i32, [vp, u64, vp, u32, ctypes.c_char_p]),
        "dash_shrink_many": (i32, [vp, vp, u64, vp, u64, vp, vp, u32, vp, ctypes.POINTER(ShrinkManyReport)]),
        "dash_shrink_assign": (i32, [vp, u64, u64, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                     ctypes.POINTER(i32)]),
        "dash_compute_addr_metrics": (i32, [vp, ctypes.POINTER(AddrTotals)]),
        "dash_read_addr_metrics": (i32, [vp, u64, u64, vp, vp]),
        "dash_addr_class": (i32, [ctypes.POINTER(AddrMetrics)]),
        "dash_addr_metrics_from_events": (i32, [vp, u64, u32, u32, vp, ctypes.POINTER(u64)]),
        "dash_set_system_delays": (i32, [vp, vp, u64]),
        "dash_delay_schedule": (i32, [u64, u32, u32, vp]),
        "dash_delay_count": (i32, [ctypes.POINTER(DelaySpace), u32, ctypes.POINTER(u64)]),
        "dash_delay_word": (i32, [ctypes.POINTER(DelaySpace), u32, u64, ctypes.POINTER(u64)]),
        "dash_explore_delays": (i32, [vp, u64, ctypes.POINTER(DelaySpace), u64, vp, u64, ctypes.POINTER(u64), vp,
                                      ctypes.POINTER(ExploreTotals)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


# handle-less entry points whose failure text dash_last_error(NULL) holds (dash.h)
_GLOBAL_MSG = ("dash_create", "dash_run_host_batched", "dash_simulate_dir", "dash_probe_box")


def _check(rc: int, what: str, handle=None):
    if rc != OK:
        msg = what
        if handle or what in _GLOBAL_MSG:
            detail = lib().dash_last_error(handle)
            if detail:
                msg = f"{what}: {detail.decode(errors='replace')}"
        raise DashError(rc, msg)


# ------------------------------------------------------------------ host boundary

def parse_core_file(path, num_procs=4, max_instr=32) -> np.ndarray:
    """initializeProcessor's parse (assignment.c:822-850) -> packed u16 records."""
    out = np.zeros(max(max_instr, 1), dtype=np.uint16)
    n = ctypes.c_uint32(0)
    _check(lib().dash_parse_core_file(str(path).encode(), num_procs, max_instr,
                                      out.ctypes.data, ctypes.byref(n)), f"parse {path}")
    return out[:n.value].copy()


def parse_core_text(data: bytes, num_procs=4, max_instr=32):
    """dash_parse_core_text: dash_parse_core_file's rules on bytes in memory. Returns (accepted
    words, rc) and does not raise on DASH_EPARSE / DASH_EADDR: the words are those accepted
    before the failing record."""
    data = bytes(data)
    out = np.zeros(max(max_instr, 1), dtype=np.uint16)
    n = ctypes.c_uint32(0)
    rc = lib().dash_parse_core_text(data, len(data), num_procs, max_instr, out.ctypes.data, ctypes.byref(n))
    return out[:n.value].copy(), rc


def pack_text(blobs):
    """One slab for dash_load_text: the blobs back to back, each on a 16-byte boundary.
    Returns (slab bytes, offsets u64, lengths u32)."""
    lengths = np.array([len(b) for b in blobs], dtype=np.uint32)
    padded = (lengths.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)
    offsets = np.zeros(len(blobs), dtype=np.uint64)
    if len(blobs):
        offsets[1:] = np.cumsum(padded)[:-1]
    slab = bytearray(int(padded.sum()))
    for b, o in zip(blobs, offsets):
        slab[int(o):int(o) + len(b)] = b
    return bytes(slab), offsets, lengths


def read_dirs_text(dirs, num_procs=4, max_instr=32, cap=None):
    """dash_read_dirs_text: (rc, need, slab bytes, offsets, lengths). cap=None measures first and
    reads into a buffer of exactly `need` bytes; cap=k reads into a buffer of k bytes."""
    arr = (ctypes.c_char_p * max(len(dirs), 1))(*[str(d).encode() for d in dirs])
    nf = len(dirs) * num_procs
    off = np.zeros(max(nf, 1), dtype=np.uint64)
    ln = np.zeros(max(nf, 1), dtype=np.uint32)
    need = ctypes.c_uint64(0)
    if cap is None:
        rc = lib().dash_read_dirs_text(arr, len(dirs), num_procs, max_instr, None, 0, off.ctypes.data,
                                       ln.ctypes.data, ctypes.byref(need))
        if rc != OK:
            return rc, need.value, b"", off[:nf], ln[:nf]
        cap = need.value
    buf = ctypes.create_string_buffer(max(cap, 1))
    rc = lib().dash_read_dirs_text(arr, len(dirs), num_procs, max_instr, buf, cap, off.ctypes.data,
                                   ln.ctypes.data, ctypes.byref(need))
    return rc, need.value, buf.raw[:cap], off[:nf], ln[:nf]


def init_node_state(node_id: int, cache_size=4) -> NodeState:
    s = NodeState()
    lib().dash_init_node_state(ctypes.byref(s), node_id, cache_size)
    return s


def dump_node(state: NodeState, node_id: int, cache_size=4) -> str:
    """printProcessorState (assignment.c:853-905), byte-exact."""
    buf = ctypes.create_string_buffer(16384)
    n = lib().dash_dump_node(ctypes.byref(state), node_id, cache_size, buf, 16384)
    if n < 0:
        raise DashError(n, "dump_node")
    return buf.raw[:n].decode()


def digest_node(state: NodeState, node_id: int, cache_size=4) -> int:
    return int(lib().dash_digest_node(ctypes.byref(state), node_id, cache_size))


def format_events(events, kinds=(0, 1)) -> str:
    """Lines exactly as the reference prints them under -D DEBUG_MSG / -D DEBUG_INSTR."""
    buf = ctypes.create_string_buffer(128)
    out = []
    for e in events:
        if e.kind in kinds:
            n = lib().dash_format_event(ctypes.byref(e), buf, 128)
            _check(n if n < 0 else OK, "dash_format_event")
            out.append(buf.value.decode())
    return "".join(out)


def check_states(nodes, num_procs: int, cache_size: int):
    """dash_check_states: the coherence invariants of one system's final state on the host. nodes:
    num_procs NodeState (read_state's list, or states built by hand). Returns (record dict with the
    COHERENCE_FIELDS, per-address bits uint32 [num_procs * 16])."""
    arr = (NodeState * max(len(nodes), 1))()
    for t, s in enumerate(nodes):  # any object with dash_node_state's fields
        for name, _ in NodeState._fields_:
            getattr(arr[t], name)[:] = list(getattr(s, name))
    rec = Coherence()
    bits = np.zeros(MAX_PROCS * MEM_SIZE, dtype=np.uint32)
    if len(nodes) < min(num_procs, MAX_PROCS):
        raise ValueError("check_states: fewer states than num_procs")
    _check(lib().dash_check_states(arr, num_procs, cache_size, ctypes.byref(rec), bits.ctypes.data),
           "dash_check_states")
    return {f: int(getattr(rec, f)) for f in COHERENCE_FIELDS}, bits[:num_procs * MEM_SIZE].copy()


def addr_class(record) -> int:
    """dash_addr_class: the sharing class (ADDR_UNTOUCHED .. ADDR_MULTI_WRITER) of one per-address record,
    a mapping or structured-array element with the ADDR_METRIC_FIELDS."""
    m = AddrMetrics(**{f: int(record[f]) for f in ADDR_METRIC_FIELDS})
    c = lib().dash_addr_class(ctypes.byref(m))
    _check(c if c < 0 else OK, "dash_addr_class")
    return c


def addr_metrics_from_events(events, num_procs: int, rounds: int):
    """dash_addr_metrics_from_events: the per-address records of one system from its events
    (Engine.read_events' list, or (round, node, kind, word) tuples), over the rounds < `rounds`.
    Returns (records, a structured array [num_procs * 16] with the ADDR_METRIC_FIELDS; the number of
    events whose address is num_procs * 16 or more)."""
    arr = (Event * max(len(events), 1))()
    for k, e in enumerate(events):
        arr[k] = e if isinstance(e, Event) else Event(*[int(x) for x in e])
    rec = np.zeros(max(num_procs, 0) * MEM_SIZE if num_procs <= MAX_PROCS else 0, dtype=ADDR_METRICS_DTYPE)
    out = rec if rec.size else np.zeros(1, dtype=ADDR_METRICS_DTYPE)
    foreign = ctypes.c_uint64()
    _check(lib().dash_addr_metrics_from_events(arr, len(events), num_procs, rounds, out.ctypes.data,
                                               ctypes.byref(foreign)), "dash_addr_metrics_from_events")
    return rec, foreign.value


def seed_schedule(seed: int, num_procs: int, rounds: int) -> np.ndarray:
    """dash_seed_schedule: the seeded schedule of `seed` as a set_schedule table, uint8
    [rounds][num_procs] of SIT_OUT or the node's delivery position (seed 0: lockstep rounds)."""
    sched = np.zeros((rounds, num_procs), dtype=np.uint8)
    # a zero-round table still needs a non-null pointer
    buf = sched if rounds and num_procs else np.zeros(1, dtype=np.uint8)
    _check(lib().dash_seed_schedule(seed, num_procs, rounds, buf.ctypes.data), "dash_seed_schedule")
    return sched


def delay_pack(delays) -> int:
    """A delay word (dash_set_system_delays) from up to four (node, start, length) delays: node 0..7,
    start round 0..1022, length a power of two 1..128; slot s holds delays[s], the others are empty."""
    delays = list(delays)
    if len(delays) > 4:
        raise ValueError("delay_pack: at most four delays")
    word = DELAY_LOCKSTEP
    for s, (t, r, length) in enumerate(delays):
        t, r, length = int(t), int(r), int(length)
        e = length.bit_length() - 1
        if not (0 <= t < 8 and 0 <= r <= 1022 and 1 <= length <= 128 and length == 1 << e):
            raise ValueError(f"delay_pack: delay {(t, r, length)} out of range")
        word = word & ~(0xFFFF << (16 * s)) | (t | e << 3 | r << 6) << (16 * s)
    return word


def delay_unpack(word: int) -> list:
    """The non-empty slots of a delay word as (node, start, length), in slot order."""
    slots = [(int(word) >> (16 * s)) & 0xFFFF for s in range(4)]
    return [(f & 7, f >> 6, 1 << ((f >> 3) & 7)) for f in slots if f != DELAY_EMPTY]


def delay_format(word: int) -> str:
    """A delay word in the CLI's spelling, t@r+len[,t@r+len..] (cache_simulator --delays); lockstep is ''."""
    return ",".join(f"{t}@{r}+{n}" for t, r, n in delay_unpack(word))


def _delay_space(starts: int, lens: int, max_delays: int) -> DelaySpace:
    if min(starts, lens, max_delays) < 0 or max(starts, lens, max_delays) > 0xFFFFFFFF:
        raise DashError(EINVAL, "dash_delay_space")
    return DelaySpace(starts, lens, max_delays, 0)


def delay_count(starts: int, lens: int, max_delays: int, num_procs: int) -> int:
    """dash_delay_count: K, the schedules of the space lockstep + at most max_delays delays with start
    rounds 0 .. starts - 1 and lengths 1 .. 2^(lens - 1), over num_procs nodes."""
    K = ctypes.c_uint64()
    _check(lib().dash_delay_count(ctypes.byref(_delay_space(starts, lens, max_delays)), num_procs, ctypes.byref(K)),
           "dash_delay_count")
    return K.value


def delay_word(starts: int, lens: int, max_delays: int, num_procs: int, index: int) -> int:
    """dash_delay_word: the delay word of schedule `index` < delay_count(...) (index 0 is lockstep,
    indices rise with the delay count)."""
    w = ctypes.c_uint64()
    _check(lib().dash_delay_word(ctypes.byref(_delay_space(starts, lens, max_delays)), num_procs, index,
                                 ctypes.byref(w)), "dash_delay_word")
    return w.value


def delay_schedule(word: int, num_procs: int, rounds: int) -> np.ndarray:
    """dash_delay_schedule: the rounds [0, rounds) of a delay word as a set_schedule table, uint8
    [rounds][num_procs] of SIT_OUT or the node's own position."""
    sched = np.zeros((rounds, num_procs), dtype=np.uint8)
    buf = sched if rounds and num_procs else np.zeros(1, dtype=np.uint8)
    _check(lib().dash_delay_schedule(word, num_procs, rounds, buf.ctypes.data), "dash_delay_schedule")
    return sched


def pack_weights(weights) -> int:
    """Per-node weights (each 0..31, node t first) as dash_set_micro_seeds' 64-bit vector; None =
    uniform; an int is passed through."""
    if weights is None:
        return MICRO_UNIFORM
    if isinstance(weights, (int, np.integer)):
        return int(weights)
    w = [int(x) for x in weights]
    if len(w) > MAX_PROCS or any(x < 0 or x > 255 for x in w):
        raise ValueError("weights: at most 8 values of one byte each")
    return sum(x << (8 * t) for t, x in enumerate(w))


def micro_pick(seed: int, round: int, enabled: int, weights, num_procs: int) -> int:
    """dash_micro_pick: the node that acts in `round` of the seeded micro-step schedule (seed,
    weights) when the nodes in the bit set `enabled` are enabled."""
    t = lib().dash_micro_pick(seed, round, enabled, pack_weights(weights), num_procs)
    _check(t if t < 0 else OK, "dash_micro_pick")
    return t


def explore_assign(S: int, G: int, K: int, F: int, pass_: int, k: int):
    """dash_explore_assign: (source, seed, counted) of system k in pass `pass_` of an explore_sources
    call with G sources and K seeds per source from F on a handle of S systems."""
    src, seed, counted = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_int()
    _check(lib().dash_explore_assign(S, G, K, F, pass_, k, ctypes.byref(src), ctypes.byref(seed),
                                     ctypes.byref(counted)), "dash_explore_assign")
    return src.value, seed.value, bool(counted.value)


def shrink_candidate(lens, c: int):
    """dash_shrink_candidate: (C, node, start, count) of candidate c of a shrink round over a base with
    lens[t] instructions on node t: C candidates in all, and candidate c deletes instructions
    [start, start + count) of `node`. C == 0 (an empty base) returns (0, None, None, None); c >= C > 0
    raises DashError(EINVAL)."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    assert lens.ndim == 1
    node, start, count = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    C = lib().dash_shrink_candidate(lens.ctypes.data, len(lens), c, ctypes.byref(node), ctypes.byref(start),
                                    ctypes.byref(count))
    _check(C if C < 0 else OK, "dash_shrink_candidate")
    return (C, node.value, start.value, count.value) if C else (0, None, None, None)


def shrink_assign(cands, S: int, pass_: int, k: int):
    """dash_shrink_assign: (job, cand, counted) of system k in sub-pass `pass_` of a shrink_many round whose
    jobs have cands[i] candidates, on a handle of S systems; an uncounted system holds the base of job
    k % len(cands)."""
    cands = np.ascontiguousarray(cands, dtype=np.uint64)
    assert cands.ndim == 1
    job, cand, counted = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    _check(lib().dash_shrink_assign(cands.ctypes.data if len(cands) else None, len(cands), S, pass_, k,
                                    ctypes.byref(job), ctypes.byref(cand), ctypes.byref(counted)), "dash_shrink_assign")
    return job.value, cand.value, bool(counted.value)


def write_dir(trace, lens, out_dir):
    """dash_write_dir: one trace set (trace [num_procs, stride] u16, lens [num_procs]) as
    out_dir/core_<n>.txt in the fixtures' format; parse_core_file reads the same words back."""
    trace = np.ascontiguousarray(trace, dtype=np.uint16)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    assert trace.ndim == 2 and lens.shape == (trace.shape[0],)
    buf = trace if trace.size else np.zeros(1, dtype=np.uint16)
    _check(lib().dash_write_dir(buf.ctypes.data, trace.shape[1], lens.ctypes.data, trace.shape[0],
                                str(out_dir).encode()), f"dash_write_dir {out_dir}")


def probe_box(device=0) -> dict:
    """dash_probe_box: device identity and clock limits, and a fixed VALU probe with the shader
    clock the box held while it ran (a benchmark line's box description)."""
    b = BoxProbe()
    _check(lib().dash_probe_box(device, ctypes.byref(b)), "dash_probe_box")
    d = {f: getattr(b, f) for f, _ in BoxProbe._fields_}
    d["name"], d["arch"] = b.name.decode(errors="replace"), b.arch.decode(errors="replace")
    return d


def simulate_dir(test_dir, out_dir=".", num_procs=4, cache_size=4, max_instr=32, device=0) -> dict:
    """main() end to end for one trace directory (assignment.c:126-739)."""
    st = Stats()
    _check(lib().dash_simulate_dir(str(test_dir).encode(), num_procs, cache_size, max_instr,
                                   str(out_dir).encode(), device, ctypes.byref(st)),
           f"simulate_dir {test_dir}")
    return st.as_dict()


def run_host_batched(packed: np.ndarray, lens: np.ndarray, batches: int, num_procs=8, cache_size=4,
                     max_instr=None, device=0, flags=0):
    """dash_run_host_batched: host traces [systems, num_procs, stride] u16 in `batches` batches
    on two handles, copies overlapped with runs. Returns (stats dict, digests, rounds, errors)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint16)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    nsys = packed.shape[0]
    assert packed.ndim == 3 and packed.shape[1] == num_procs and lens.shape == (nsys, num_procs)
    cfg = Cfg(num_procs, cache_size, max_instr or packed.shape[2], flags, nsys, 0, device, 0, 0)
    st = Stats()
    d = np.zeros(nsys, dtype=np.uint64)
    r = np.zeros(nsys, dtype=np.uint32)
    e = np.zeros(nsys, dtype=np.uint32)
    _check(lib().dash_run_host_batched(ctypes.byref(cfg), packed.ctypes.data, packed.shape[2], lens.ctypes.data,
                                       nsys, batches, ctypes.byref(st), d.ctypes.data, r.ctypes.data,
                                       e.ctypes.data), "dash_run_host_batched")
    return st.as_dict(), d, r, e


# ------------------------------------------------------------------ device engine

class Engine:
    """One batch of independent N-node systems on one GPU (a dash_t handle)."""

    def __init__(self, num_systems, num_procs=8, cache_size=4, max_instr=32, keep_state=False,
                 device=0, max_rounds=0, flags=0, trace_events=0, schedule_seed=0):
        self.cfg = Cfg(num_procs, cache_size, max_instr, (KEEP_STATE if keep_state else 0) | flags,
                       num_systems, max_rounds, device, trace_events, schedule_seed)
        self.h = ctypes.c_void_p()
        _check(lib().dash_create(ctypes.byref(self.cfg), ctypes.byref(self.h)), "dash_create")
        self.num_systems = num_systems
        self.num_procs = num_procs
        self.cache_size = cache_size

    def close(self):
        if self.h:
            lib().dash_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_traces(self, packed: np.ndarray, lens: np.ndarray):
        """packed: [systems, num_procs, stride] u16; lens: [systems, num_procs] u32."""
        packed = np.ascontiguousarray(packed, dtype=np.uint16)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        assert packed.ndim == 3 and packed.shape[:2] == (self.num_systems, self.num_procs)
        assert lens.shape == (self.num_systems, self.num_procs)
        _check(lib().dash_load_traces(self.h, packed.ctypes.data, packed.shape[2], lens.ctypes.data,
                                      self.num_systems), "dash_load_traces", self.h)

    def load_dir(self, test_dir):
        _check(lib().dash_load_dir(self.h, str(test_dir).encode(), 0), "dash_load_dir", self.h)

    def load_dirs(self, dirs, device=False):
        """Bulk ingest: system k = trace directory dirs[k]. device=True parses the text on the
        GPU (dash_load_dirs_device); after a failure of that path the handle is not loaded."""
        arr = (ctypes.c_char_p * max(len(dirs), 1))(*[str(d).encode() for d in dirs])
        if device:
            _check(lib().dash_load_dirs_device(self.h, arr, len(dirs)), "dash_load_dirs_device", self.h)
        else:
            _check(lib().dash_load_dirs(self.h, arr, len(dirs)), "dash_load_dirs", self.h)

    def load_text(self, blobs):
        """dash_load_text: blobs[system][node] = the bytes of that node's core_<n>.txt, parsed on
        the GPU straight into the simulator's layout."""
        flat = [bytes(b) for row in blobs for b in row]
        assert len(blobs) == self.num_systems and len(flat) == self.num_systems * self.num_procs
        self.load_text_slab(*pack_text(flat))

    def load_text_slab(self, slab: bytes, offsets, lengths):
        """dash_load_text on a caller-laid-out slab: file sys * num_procs + node is
        slab[offsets[f] : offsets[f] + lengths[f]] (any alignment)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        assert offsets.shape == lengths.shape == (self.num_systems * self.num_procs,)
        assert not len(offsets) or int((offsets + lengths.astype(np.uint64)).max()) <= len(slab)
        slab = bytes(slab)  # read in place by the call (no copy for a bytes object)
        ptr = ctypes.cast(ctypes.c_char_p(slab), ctypes.c_void_p)
        _check(lib().dash_load_text(self.h, ptr, offsets.ctypes.data, lengths.ctypes.data, len(offsets)),
               "dash_load_text", self.h)

    def read_traces(self):
        """dash_read_traces: (packed [systems, num_procs, max_instr] u16, lens [systems, num_procs])
        as the device holds them; words at or past a node's length read as 0."""
        stride = max(int(self.cfg.max_instr), 1)
        packed = np.zeros((self.num_systems, self.num_procs, stride), dtype=np.uint16)
        lens = np.zeros((self.num_systems, self.num_procs), dtype=np.uint32)
        _check(lib().dash_read_traces(self.h, packed.ctypes.data, stride, lens.ctypes.data), "dash_read_traces",
               self.h)
        return packed, lens

    def ingest_info(self) -> dict:
        """dash_ingest_info: the last load_text / load_dirs(device=True) as numbers."""
        r = IngestReport()
        _check(lib().dash_ingest_info(self.h, ctypes.byref(r)), "dash_ingest_info", self.h)
        d = {f: getattr(r, f) for f, _ in IngestReport._fields_}
        d["system"], d["node"] = divmod(int(r.file), self.num_procs)
        return d

    def dump_system(self, sys: int, out_dir):
        _check(lib().dash_dump_system(self.h, sys, str(out_dir).encode()), "dash_dump_system", self.h)

    def write_digests(self, path):
        _check(lib().dash_write_digests(self.h, str(path).encode()), "dash_write_digests", self.h)

    def generate(self, seed, length, kind=GEN_UNIFORM, locality=0, sys_base=0):
        g = Gen(seed, sys_base, kind, locality, length, 0)
        _check(lib().dash_generate(self.h, ctypes.byref(g)), "dash_generate", self.h)

    def set_schedule(self, sched: np.ndarray):
        """dash_set_schedule: an explicit round schedule, uint8 [rounds][num_procs] (SIT_OUT or
        the node's delivery position); later rounds are lockstep. Needs schedule_seed != 0."""
        sched = np.ascontiguousarray(sched, dtype=np.uint8)
        assert sched.ndim == 2 and sched.shape[1] == self.num_procs
        _check(lib().dash_set_schedule(self.h, sched.ctypes.data, sched.shape[0]), "dash_set_schedule", self.h)

    def set_micro_schedule(self, acts: np.ndarray):
        """dash_set_micro_schedule: uint8 [rounds][num_procs] of SIT_OUT / MICRO_STEP / MICRO_SEND,
        at most one acting node per round (include/dash.h). Needs schedule_seed != 0."""
        acts = np.ascontiguousarray(acts, dtype=np.uint8)
        assert acts.ndim == 2 and acts.shape[1] == self.num_procs
        _check(lib().dash_set_micro_schedule(self.h, acts.ctypes.data, acts.shape[0]), "dash_set_micro_schedule",
               self.h)

    def set_system_seeds(self, seeds):
        """dash_set_system_seeds: system k follows the seeded schedule of seeds[k] (0 = lockstep);
        None returns the handle to its own seed. Needs schedule_seed != 0."""
        if seeds is None:
            _check(lib().dash_set_system_seeds(self.h, None, 0), "dash_set_system_seeds", self.h)
            return
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.ndim == 1
        _check(lib().dash_set_system_seeds(self.h, seeds.ctypes.data, len(seeds)), "dash_set_system_seeds", self.h)

    def set_system_delays(self, words):
        """dash_set_system_delays: system k follows the delay word words[k] (delay_pack; DELAY_LOCKSTEP
        = lockstep); None returns the handle to its own seed. Needs schedule_seed != 0."""
        if words is None:
            _check(lib().dash_set_system_delays(self.h, None, 0), "dash_set_system_delays", self.h)
            return
        words = np.ascontiguousarray(words, dtype=np.uint64)
        assert words.ndim == 1
        _check(lib().dash_set_system_delays(self.h, words.ctypes.data, len(words)), "dash_set_system_delays", self.h)

    def set_micro_seeds(self, seeds, weights=None, weights_per_system=None):
        """dash_set_micro_seeds: system k follows the seeded micro-step schedule of seeds[k] under
        its weight vector. weights: one vector for every system, a sequence of per-node weights or a
        packed int (pack_weights); weights_per_system: one packed uint64 per system instead; neither
        = uniform. seeds None returns the handle to its own seed. Needs schedule_seed != 0."""
        if seeds is None:
            _check(lib().dash_set_micro_seeds(self.h, None, None, 0), "dash_set_micro_seeds", self.h)
            return
        if weights is not None and weights_per_system is not None:
            raise ValueError("set_micro_seeds: weights or weights_per_system, not both")
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.ndim == 1
        if weights is not None:
            weights_per_system = np.full(len(seeds), pack_weights(weights), dtype=np.uint64)
        wp = None
        if weights_per_system is not None:
            weights_per_system = np.ascontiguousarray(weights_per_system, dtype=np.uint64)
            assert weights_per_system.shape == seeds.shape
            wp = weights_per_system.ctypes.data
        _check(lib().dash_set_micro_seeds(self.h, seeds.ctypes.data, wp, len(seeds)), "dash_set_micro_seeds", self.h)

    def read_micro_acts(self, sys: int) -> np.ndarray:
        """dash_read_micro_acts: the schedule system `sys` followed in the last run under micro
        seeds, uint8 [rounds][num_procs] as set_micro_schedule takes it (needs trace_events)."""
        n = ctypes.c_uint32()
        rc = lib().dash_read_micro_acts(self.h, sys, None, 0, ctypes.byref(n))
        if rc != EINVAL or n.value == 0:  # EINVAL with the rounds set: the table's size
            _check(rc, "dash_read_micro_acts", self.h)
        acts = np.zeros((n.value, self.num_procs), dtype=np.uint8)
        if n.value:
            _check(lib().dash_read_micro_acts(self.h, sys, acts.ctypes.data, n.value, ctypes.byref(n)),
                   "dash_read_micro_acts", self.h)
        return acts

    def explore_micro(self, src: int, first_seed: int, num_seeds: int, weights=None, cap=None) -> list:
        """dash_explore_micro: explore() over seeded micro-step schedules, seeds first_seed + i under
        one weight vector (None = uniform)."""
        return self._explore(lib().dash_explore_micro, "dash_explore_micro", cap, src, first_seed, num_seeds,
                             pack_weights(weights))

    def broadcast_system(self, src: int):
        """dash_broadcast_system: every system becomes a copy of system src (on the device)."""
        _check(lib().dash_broadcast_system(self.h, src), "dash_broadcast_system", self.h)

    def explore(self, src: int, first_seed: int, num_seeds: int, cap=None) -> list:
        """dash_explore: the distinct outcomes of system src under seeds first_seed + i, i <
        num_seeds, as dicts (digest, count, seed = the lowest seed that reached it, rounds and errors
        of that witness), in witness-seed order. cap=k returns the first k; the total is
        explore_total afterwards either way."""
        return self._explore(lib().dash_explore, "dash_explore", cap, src, first_seed, num_seeds)

    def _explore(self, fn, what, cap, *args) -> list:
        n = ctypes.c_uint32()
        want = 1024 if cap is None else cap
        while True:
            arr = (Outcome * max(want, 1))()
            _check(fn(self.h, *args, arr, want, ctypes.byref(n)), what, self.h)
            if cap is not None or n.value <= want:
                break
            want = n.value  # more outcomes than the first guess held: once more, with room for all
        cap = want
        self.explore_total = int(n.value)
        return [{f: int(getattr(o, f)) for f, _ in Outcome._fields_} for o in arr[:min(n.value, cap)]]

    def explore_sources(self, num_sources: int, first_seed: int, seeds_per_source: int, weights=None,
                        table_slots=0, cap=None):
        """dash_explore_sources: systems 0 .. num_sources - 1 are the sources; every one runs
        seeds_per_source schedules from first_seed (weights None: seeded round schedules; else seeded
        micro-step schedules under that vector, MICRO_UNIFORM for uniform). Returns (outcomes, a
        structured array with OUTCOME_EX_DTYPE ordered by (source, witness seed); per_source, one
        SOURCE_SUMMARY_DTYPE record per source; totals dict). cap=k keeps the first k outcomes. The
        result also stays on the engine as explore_sources_result; when the table filled it is stored
        there before DashError(ETRUNC) is raised."""
        want = min(max(num_sources * seeds_per_source, 1), 1 << 22) if cap is None else cap
        w = None if weights is None else ctypes.byref(ctypes.c_uint64(pack_weights(weights)))
        fn = lib().dash_explore_sources
        return self._explore_sources("dash_explore_sources", num_sources, want, cap, lambda *res: fn(
            self.h, num_sources, first_seed, seeds_per_source, w, table_slots, *res))

    def explore_delays(self, num_sources: int, starts: int, lens: int, max_delays: int, table_slots=0, cap=None):
        """dash_explore_delays: explore_sources over every schedule within max_delays delays of lockstep
        (start rounds 0 .. starts - 1, lengths 1 .. 2^(lens - 1); delay_count gives their number). The
        outcomes' seed is the lowest schedule index that reached them, a fewest-delays witness:
        delay_word turns it into the delay word, delay_unpack into (node, start, length). The result is
        explore_sources' and stays on the engine the same way."""
        space = _delay_space(starts, lens, max_delays)
        want = 4096 if cap is None else cap
        fn = lib().dash_explore_delays
        return self._explore_sources("dash_explore_delays", num_sources, want, cap, lambda *res: fn(
            self.h, num_sources, ctypes.byref(space), table_slots, *res))

    def _explore_sources(self, what, num_sources, want, cap, call):
        per = np.zeros(max(num_sources, 0), dtype=SOURCE_SUMMARY_DTYPE)
        per_buf = per if per.size else np.zeros(1, dtype=SOURCE_SUMMARY_DTYPE)
        while True:
            outs = np.zeros(max(want, 1), dtype=OUTCOME_EX_DTYPE)
            tot, n = ExploreTotals(), ctypes.c_uint64()
            rc = call(outs.ctypes.data, want, ctypes.byref(n), per_buf.ctypes.data, ctypes.byref(tot))
            if rc not in (OK, ETRUNC) or cap is not None or n.value <= want:
                break
            want = n.value  # more outcomes than the first guess held: once more, with room for all
        if rc in (OK, ETRUNC):
            self.explore_total = int(n.value)
            self.explore_sources_result = (outs[:min(n.value, want)], per, tot.as_dict())
        _check(rc, what, self.h)
        return self.explore_sources_result

    def shrink(self, src: int, coh_all: int, err_all=0, err_none=0xFFFFFFFF, seed=0, cap=None) -> dict:
        """dash_shrink: system src cut down, on the GPU, to a 1-minimal trace set whose final state still
        has the coherence bits coh_all, the error bits err_all and none of err_none, under the lockstep
        schedule (seed 0) or the seeded round schedule `seed`. Returns dict(trace [num_procs, max_instr]
        u16, lens [num_procs], steps: one SHRINK_STEP_DTYPE record per round (the winner and the base's
        candidate count), report dict). Afterwards every system holds the minimal set, run and checked.
        cap=k keeps the first k steps (report["rounds"] has their number). The library runs it as the
        one-job case of shrink_many's engine; a source that does not meet the goal is an error here."""
        goal = ShrinkGoal(coh_all, err_all, err_none, 0)
        stride = max(int(self.cfg.max_instr), 1)
        trace = np.zeros((self.num_procs, stride), dtype=np.uint16)
        lens = np.zeros(self.num_procs, dtype=np.uint32)
        # every round deletes at least one instruction, so a source has at most as many rounds as
        # instructions (the call cannot be repeated for a longer list: it leaves the minimal set behind)
        want = min(self.num_procs * stride, 1 << 20) if cap is None else cap
        steps = np.zeros(max(want, 1), dtype=SHRINK_STEP_DTYPE)
        n, rep = ctypes.c_uint32(), ShrinkReport()
        _check(lib().dash_shrink(self.h, src, seed, ctypes.byref(goal), trace.ctypes.data, stride, lens.ctypes.data,
                                 steps.ctypes.data, want, ctypes.byref(n), ctypes.byref(rep)), "dash_shrink", self.h)
        return {"trace": trace, "lens": lens, "steps": steps[:min(n.value, want)], "report": rep.as_dict()}

    def shrink_many(self, jobs, cap=None) -> dict:
        """dash_shrink_many: the jobs, rows of (src, seed, coh_all, err_all, err_none), shrunk side by side
        on the GPU, each to where Engine.shrink (the same engine with one job) takes it alone. Returns dict(trace [J, num_procs,
        max_instr] u16, lens [J, num_procs], steps: a list of SHRINK_STEP_DTYPE arrays, results: a
        SHRINK_RESULT_DTYPE array (status SHRINK_MINIMAL or SHRINK_UNMET per job), report dict).
        Afterwards system k holds the final set of job k % J, run and checked. cap=k keeps the first k
        steps of every job (results["rounds"] has their number)."""
        rows = [tuple(int(x) for x in j) for j in jobs]
        rec = np.zeros(len(rows), dtype=SHRINK_JOB_DTYPE)
        for i, (src, seed, coh_all, err_all, err_none) in enumerate(rows):
            rec[i] = (src, seed, coh_all, err_all, err_none, 0)
        J, N, stride = len(rows), self.num_procs, max(int(self.cfg.max_instr), 1)
        trace = np.zeros((J, N, stride), dtype=np.uint16)
        lens = np.zeros((J, N), dtype=np.uint32)
        want = N * stride if cap is None else cap  # a job has at most as many rounds as instructions
        steps = np.zeros((max(J, 1), max(want, 1)), dtype=SHRINK_STEP_DTYPE)
        results = np.zeros(max(J, 1), dtype=SHRINK_RESULT_DTYPE)
        rep = ShrinkManyReport()
        _check(lib().dash_shrink_many(self.h, rec.ctypes.data if J else None, J, trace.ctypes.data, stride,
                                      lens.ctypes.data, steps.ctypes.data if want else None, want, results.ctypes.data,
                                      ctypes.byref(rep)), "dash_shrink_many", self.h)
        return {"trace": trace, "lens": lens, "steps": [steps[i, :min(int(results["rounds"][i]), want)] for i in range(J)],
                "results": results[:J], "report": rep.as_dict()}

    def run(self) -> dict:
        st = Stats()
        _check(lib().dash_run(self.h, ctypes.byref(st)), "dash_run", self.h)
        return st.as_dict()

    def read_state(self, sys: int):
        arr = (NodeState * self.num_procs)()
        _check(lib().dash_read_state(self.h, sys, arr), "dash_read_state", self.h)
        return list(arr)

    def write_states(self, first: int, systems):
        """dash_test_write_states (testing only): overwrite the kept states of systems first ..
        first + len(systems) - 1; systems is a list of lists of num_procs node states (any objects
        with dash_node_state's fields). The coherence records become invalid; everything else the
        run left (digests, rounds, errors, histograms, events, metrics) stays and no longer
        describes the state."""
        arr = (NodeState * max(len(systems) * self.num_procs, 1))()
        for k, nodes in enumerate(systems):
            if len(nodes) != self.num_procs:
                raise ValueError("write_states: a system needs num_procs node states")
            for t, s in enumerate(nodes):
                for name, _ in NodeState._fields_:
                    getattr(arr[k * self.num_procs + t], name)[:] = list(getattr(s, name))
        _check(lib().dash_test_write_states(self.h, first, len(systems), arr), "dash_test_write_states", self.h)

    def read_hist(self, sys: int) -> np.ndarray:
        h = np.zeros(NUM_TXN, dtype=np.uint32)
        _check(lib().dash_read_hist(self.h, sys, h.ctypes.data), "dash_read_hist", self.h)
        return h

    def read_results(self, first=0, count=None):
        count = self.num_systems - first if count is None else count
        d = np.zeros(count, dtype=np.uint64)
        r = np.zeros(count, dtype=np.uint32)
        e = np.zeros(count, dtype=np.uint32)
        _check(lib().dash_read_results(self.h, first, count, d.ctypes.data, r.ctypes.data,
                                       e.ctypes.data), "dash_read_results", self.h)
        return d, r, e

    def read_events(self, sys: int) -> list:
        """The system's DEBUG_MSG / DEBUG_INSTR events in lockstep order (needs trace_events)."""
        n = ctypes.c_uint32()
        # count first (cap 0), then read exactly that many: the log keeps trace_events rounded up to
        # a multiple of 4 rounds, so trace_events * num_procs can undercount it
        _check(lib().dash_read_events(self.h, sys, None, 0, ctypes.byref(n)), "dash_read_events", self.h)
        cap = n.value
        arr = (Event * max(cap, 1))()
        _check(lib().dash_read_events(self.h, sys, arr, cap, ctypes.byref(n)), "dash_read_events", self.h)
        return list(arr[:min(n.value, cap)])

    def compute_metrics(self) -> dict:
        """dash_compute_metrics: one GPU pass over the batch's event log of the last run (needs
        trace_events). Returns the totals: every METRIC_FIELDS entry summed over all nodes (wait_max:
        the maximum), systems and truncated_systems. The per-node records stay on the device for
        read_metrics until the next run."""
        t = MetricsTotals()
        _check(lib().dash_compute_metrics(self.h, ctypes.byref(t)), "dash_compute_metrics", self.h)
        return {f: int(getattr(t, f)) for f, _ in MetricsTotals._fields_}

    def read_metrics(self, first=0, count=None):
        """dash_read_metrics: (records, truncated) of systems [first, first + count): a structured
        array [count, num_procs] with the METRIC_FIELDS, and uint8 [count], 1 where the log was
        shorter than the system's run (its metrics then cover the log's rounds only)."""
        count = self.num_systems - first if count is None else count
        rec = np.zeros((max(count, 0), self.num_procs), dtype=METRICS_DTYPE)
        cut = np.zeros(max(count, 0), dtype=np.uint8)
        # a non-null pointer also for an empty window, whose range is still checked
        out = rec if rec.size else np.zeros(1, dtype=METRICS_DTYPE)
        flags = cut if cut.size else np.zeros(1, dtype=np.uint8)
        _check(lib().dash_read_metrics(self.h, first, count, out.ctypes.data, flags.ctypes.data),
               "dash_read_metrics", self.h)
        return rec, cut

    def compute_addr_metrics(self) -> dict:
        """dash_compute_addr_metrics: one GPU pass over the batch's event log of the last run (needs
        trace_events), by address. Returns the totals: the first eleven ADDR_METRIC_FIELDS summed over all
        records, msgs_max, foreign_events, class_addrs / class_misses / class_invalidations (lists of 5 in
        ADDR_CLASS_NAMES' order), systems and truncated_systems. The records stay on the device for
        read_addr_metrics until the next run."""
        t = AddrTotals()
        _check(lib().dash_compute_addr_metrics(self.h, ctypes.byref(t)), "dash_compute_addr_metrics", self.h)
        return {f: [int(x) for x in getattr(t, f)] if f.startswith("class_") else int(getattr(t, f))
                for f, _ in AddrTotals._fields_}

    def read_addr_metrics(self, first=0, count=None):
        """dash_read_addr_metrics: (records, truncated) of systems [first, first + count): a structured
        array [count, num_procs * 16] with the ADDR_METRIC_FIELDS, indexed by address, and uint8 [count],
        1 where the log was shorter than the system's run."""
        count = self.num_systems - first if count is None else count
        rec = np.zeros((max(count, 0), self.num_procs * MEM_SIZE), dtype=ADDR_METRICS_DTYPE)
        cut = np.zeros(max(count, 0), dtype=np.uint8)
        # a non-null pointer also for an empty window, whose range is still checked
        out = rec if rec.size else np.zeros(1, dtype=ADDR_METRICS_DTYPE)
        flags = cut if cut.size else np.zeros(1, dtype=np.uint8)
        _check(lib().dash_read_addr_metrics(self.h, first, count, out.ctypes.data, flags.ctypes.data),
               "dash_read_addr_metrics", self.h)
        return rec, cut

    def check_coherence(self) -> dict:
        """dash_check_coherence: one GPU pass over the batch's final state of the last run (needs
        keep_state). Returns the totals: systems, violating_systems, violating_clean_systems (bits set
        and no DASH_ERR_* bit), addrs, and bit_systems / bit_addrs, lists of 8 in COH_NAMES' order.
        The per-system records stay on the device for read_coherence until the next run."""
        t = CoherenceTotals()
        _check(lib().dash_check_coherence(self.h, ctypes.byref(t)), "dash_check_coherence", self.h)
        return {"systems": int(t.systems), "violating_systems": int(t.violating_systems),
                "violating_clean_systems": int(t.violating_clean_systems), "addrs": int(t.addrs),
                "bit_systems": [int(x) for x in t.bit_systems], "bit_addrs": [int(x) for x in t.bit_addrs]}

    def read_coherence(self, first=0, count=None) -> np.ndarray:
        """dash_read_coherence: the records of systems [first, first + count), a structured array
        [count] with the COHERENCE_FIELDS."""
        count = self.num_systems - first if count is None else count
        rec = np.zeros(max(count, 0), dtype=COHERENCE_DTYPE)
        out = rec if rec.size else np.zeros(1, dtype=COHERENCE_DTYPE)  # non-null for an empty window
        _check(lib().dash_read_coherence(self.h, first, count, out.ctypes.data), "dash_read_coherence", self.h)
        return rec

    def check_outcomes(self, src: int, outcomes, weights=None) -> np.ndarray:
        """dash_check_outcomes: the coherence record of every outcome explore (weights None) or
        explore_micro (its weight vector; MICRO_UNIFORM for its default) returned, by re-running the
        witness seeds: a structured array [len(outcomes)] with the COHERENCE_FIELDS."""
        arr = (Outcome * max(len(outcomes), 1))(*[Outcome(**{f: o[f] for f, _ in Outcome._fields_}) for o in outcomes])
        rec = np.zeros(len(outcomes), dtype=COHERENCE_DTYPE)
        out = rec if rec.size else np.zeros(1, dtype=COHERENCE_DTYPE)
        w = None if weights is None else ctypes.byref(ctypes.c_uint64(pack_weights(weights)))
        _check(lib().dash_check_outcomes(self.h, src, arr, len(outcomes), w, out.ctypes.data),
               "dash_check_outcomes", self.h)
        return rec

    def stream(self) -> int:
        return int(lib().dash_stream(self.h) or 0)

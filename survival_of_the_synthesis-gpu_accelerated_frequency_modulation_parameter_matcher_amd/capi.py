"""ctypes binding of libsots_hip.so (include/sots_hip.h).

Thin by design: every method is one C-ABI call.  There is no CPU fallback; if the
shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsots_hip.so")

MAX_DIMS = 16
WAVETABLE_SIZE = 32768
SAMPLE_RATE = 44100

SYNTH_2OP, SYNTH_3OP_SERIES, SYNTH_TRIPLE_PAR, SYNTH_4OP_SERIES, SYNTH_GRAPH = 0, 1, 2, 3, 4
SYNTH_DIMS = {SYNTH_2OP: 4, SYNTH_3OP_SERIES: 6, SYNTH_TRIPLE_PAR: 12, SYNTH_4OP_SERIES: 8}  # the fixed voices
SYNTH_NAMES = {"2op": SYNTH_2OP, "3op_series": SYNTH_3OP_SERIES,
               "triple_parallel": SYNTH_TRIPLE_PAR, "4op_series": SYNTH_4OP_SERIES, "graph": SYNTH_GRAPH}
GRAPH_MAX_OPERATORS = 8
# operator waveforms of the graph voice (SOTS_WAVE_*): shapes cut out of the one sine table
WAVE_SINE, WAVE_HALF, WAVE_ABS, WAVE_PULSE, WAVE_EVEN, WAVE_ABS_EVEN, WAVE_SQUARE, WAVE_SAW = range(8)
WAVE_NAMES = {"sine": WAVE_SINE, "half": WAVE_HALF, "abs": WAVE_ABS, "pulse": WAVE_PULSE, "even": WAVE_EVEN,
              "absEven": WAVE_ABS_EVEN, "square": WAVE_SQUARE, "saw": WAVE_SAW}

(STAGE_INIT, STAGE_RECOMBINE, STAGE_MUTATE, STAGE_SYNTHESISE, STAGE_WINDOW, STAGE_FFT,
 STAGE_FITNESS, STAGE_SORT, STAGE_ROTATE, STAGE_FUSED_VARIATION, STAGE_FUSED_SYNTH,
 STAGE_FUSED_SPECTRAL, STAGE_SORT_TAIL, STAGE_COUNT) = range(14)
SORT_LAZY_TAIL, SORT_FULL, SORT_TOP_ONLY = 0, 1, 2
SELECT_AUTO, SELECT_TILES, SELECT_SPLITTERS = 0, 1, 2
ARITH_CPU_PATH, ARITH_DEVICE_KERNELS = 0, 1
OBJECTIVE_MAGNITUDE, OBJECTIVE_LOG_MAGNITUDE = 0, 1  # enum sots_objective
OBJECTIVE_FLOOR_MIN, OBJECTIVE_FLOOR_MAX = 1e-30, 1.0

# the reference's Benchmarker timer names, Evolutionary_Strategy_OpenCL.hpp:117
STAGE_NAMES = ["initPopulation", "recombinePopulation", "mutatePopulation", "synthesisePopulation",
               "applyWindowPopulation", "hipFFT", "fitnessPopulation", "sortPopulation",
               "rotatePopulation", "fused:recombine+mutate", "fused:synthesise+window",
               "fused:FFT+fitness", "sortPopulation:tail"]

EXPORTS = [
    "sots_create", "sots_destroy", "sots_last_error", "sots_set_stream", "sots_synchronize",
    "sots_set_target_audio", "sots_set_target_spectrum", "sots_init_population",
    "sots_write_population", "sots_read_population", "sots_read_population_other",
    "sots_write_synth", "sots_read_synth",
    "sots_stage_recombine", "sots_stage_mutate", "sots_stage_synthesise", "sots_stage_window",
    "sots_stage_fft", "sots_stage_fitness", "sots_stage_sort", "sots_stage_select", "sots_stage_rotate",
    "sots_set_sort_mode",
    "sots_set_select_plan", "sots_select_splitter_count", "sots_write_select_splitters", "sots_read_select_splitters",
    "sots_stage_bucket_fitness", "sots_read_select_lists",
    "sots_set_synth_arithmetic", "sots_set_survivors", "sots_get_survivors", "sots_batch_set_survivors",
    "sots_execute_generation", "sots_execute_generations", "sots_get_generation",
    "sots_set_generation", "sots_timing_enable", "sots_timing_reset", "sots_stage_time_ms",
    "sots_stage_launch_times_ms",
    "sots_pack_elites_device", "sots_inject_immigrants_device", "sots_inject_gathered_device", "sots_fuse_exchange_next_sort",
    "sots_pack_elites_host",
    "sots_inject_immigrants_host", "sots_get_info",
    "sots_group_create", "sots_group_destroy", "sots_group_last_error", "sots_group_size", "sots_group_uses_rccl",
    "sots_group_island", "sots_group_set_target_audio", "sots_group_set_target_spectrum", "sots_group_init_population",
    "sots_group_execute_generations", "sots_group_synchronize", "sots_group_best",
    "sots_batch_create", "sots_batch_destroy", "sots_batch_last_error", "sots_batch_synchronize",
    "sots_batch_set_target_audio", "sots_batch_set_target_spectra", "sots_batch_init_population",
    "sots_batch_execute_generations", "sots_batch_set_synth_arithmetic", "sots_batch_read_best",
    "sots_batch_read_population",
    "sots_track", "sots_read_best_ever", "sots_read_history", "sots_stop_rule_holds", "sots_execute_until",
    "sots_batch_track", "sots_batch_read_best_ever", "sots_batch_read_history", "sots_batch_execute_until",
    "sots_batch_queue_targets_spectra", "sots_batch_queue_targets_audio", "sots_batch_queue_run", "sots_batch_queue_results",
    "sots_batch_queue_read_kept_population", "sots_queue_makespan",
    "sots_set_objective", "sots_get_objective", "sots_batch_set_objective", "sots_group_set_objective",
    "sots_set_objective_weights", "sots_get_objective_weights", "sots_batch_set_objective_weights",
    "sots_group_set_objective_weights",
    "sots_render_overlap_add", "sots_batch_set_target_audio_hop", "sots_batch_queue_targets_audio_hop",
    "sots_render_continuous", "sots_render_graph_continuous", "sots_render_graph_feedback", "sots_render_graph_genes",
    "sots_batch_queue_set_carry", "sots_batch_queue_get_carry",
    "sots_batch_set_analysis", "sots_batch_get_analysis", "sots_batch_analyse_audio_hop", "sots_batch_queue_score_audio_hop",
    "sots_create_graph", "sots_batch_create_graph", "sots_get_voice_graph",
    "sots_set_voice_waveforms", "sots_get_voice_waveforms", "sots_batch_set_voice_waveforms", "sots_batch_get_voice_waveforms",
    "sots_set_voice_feedback", "sots_get_voice_feedback", "sots_batch_set_voice_feedback", "sots_batch_get_voice_feedback",
    "sots_create_graph_genes", "sots_batch_create_graph_genes", "sots_get_voice_feedback_genes", "sots_batch_get_voice_feedback_genes",
    "sots_set_graph_synth_form", "sots_get_graph_synth_form", "sots_batch_set_graph_synth_form", "sots_batch_get_graph_synth_form",
    "sots_graph_time_parallel_capacity",
]
GRAPH_FORM_AUTO, GRAPH_FORM_LANES, GRAPH_FORM_TIME_PARALLEL = 0, 1, 2  # enum sots_graph_synth_form
GRAPH_FORM_NAMES = {"auto": GRAPH_FORM_AUTO, "lanes": GRAPH_FORM_LANES, "timeParallel": GRAPH_FORM_TIME_PARALLEL}
ANALYSIS_HOST, ANALYSIS_DEVICE = 0, 1  # enum sots_analysis
QUEUE_NO_CHUNK = 0xFFFFFFFF
RENDER_WINDOWED = 1
RENDER_GLIDE = 1
CHAIN_LIBRARY, CHAIN_SERIAL, CHAIN_RELAX = 0, 1, 2  # sots_render_graph_feedback_args.chain_form
TRACK_BEST_EVER, TRACK_HISTORY = 1, 2
BATCH_MAX_POPULATION = 1024
GROUP_OVERLAP, GROUP_FORCE_RCCL, GROUP_UNFUSED, GROUP_EVENT_WAITS = 1, 2, 4, 8
MAX_GROUP_DEVICES = 16


class SotsError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libsots_hip error {code}: {text}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_parents", C.c_uint32), ("num_offspring", C.c_uint32),
        ("num_dimensions", C.c_uint32), ("audio_length_log2", C.c_uint32),
        ("num_generations", C.c_uint32), ("synth_kind", C.c_uint32), ("workgroup_size", C.c_uint32),
        ("device", C.c_int32), ("gid_base", C.c_uint32), ("seed", C.c_uint64),
        ("param_min", C.c_float * MAX_DIMS), ("param_max", C.c_float * MAX_DIMS),
    ]


class VoiceGraph(C.Structure):
    """sots_voice_graph: the topology of the operator-graph voice (SYNTH_GRAPH)"""
    _fields_ = [("struct_size", C.c_uint32), ("num_operators", C.c_uint32), ("carriers", C.c_uint32),
                ("modulators", C.c_uint32 * GRAPH_MAX_OPERATORS)]


def _mask(bits):
    """a bit mask from an int or from a list of operator indices"""
    if isinstance(bits, int):
        return bits
    m = 0
    for i in bits:
        m |= 1 << int(i)
    return m


def make_voice_graph(operators, modulators, carriers):
    """modulators[j]: the operators that modulate operator j, carriers: the operators that are heard; each a list of
    indices or a bit mask.  Nothing is checked here: the library's rule refuses a malformed graph with its own text."""
    g = VoiceGraph()
    g.struct_size = C.sizeof(VoiceGraph)
    g.num_operators = operators
    g.carriers = _mask(carriers) & 0xFFFFFFFF
    for j, m in enumerate(list(modulators)[:GRAPH_MAX_OPERATORS]):
        g.modulators[j] = _mask(m) & 0xFFFFFFFF
    return g


def as_voice_graph(graph):
    """None, a VoiceGraph, or the JSON form {"operators": n, "modulators": [[...], ...], "carriers": [...]}"""
    if graph is None or isinstance(graph, VoiceGraph):
        return graph
    return make_voice_graph(graph["operators"], graph["modulators"], graph["carriers"])


def graph_time_parallel_capacity(graph):
    """(individuals per workgroup, levels) of the graph voice's time-parallel synthesis form for this graph
    (sots_graph_time_parallel_capacity: host only, no device needed); the library's rule refuses a malformed graph"""
    cap, levels = C.c_uint32(), C.c_uint32()
    L = load()
    rc = L.sots_graph_time_parallel_capacity(C.byref(as_voice_graph(graph)), C.byref(cap), C.byref(levels))
    if rc != 0:
        raise SotsError(rc, L.sots_last_error(None).decode())
    return cap.value, levels.value


def _waveform_codes(waveforms):
    """(pointer, count) of sots_set_voice_waveforms from None (all sine) or one code or WAVE_NAMES name per operator.
    Nothing else is checked here: the library's rule refuses with its own text."""
    if waveforms is None:
        return None, 0
    codes = [WAVE_NAMES[w] if isinstance(w, str) else int(w) for w in waveforms]
    return (C.c_uint32 * len(codes))(*[c & 0xFFFFFFFF for c in codes]), len(codes)


def _feedback_indices(feedback):
    """(pointer, count) of sots_set_voice_feedback from None (no feedback) or one index per operator.  Nothing is checked
    here: the library's rule refuses with its own text."""
    if feedback is None:
        return None, 0
    index = [float(b) for b in feedback]
    return (C.c_float * len(index))(*index), len(index)


def synth_dims(synth_kind, graph=None, feedback_genes=None):
    """genes of a voice: the fixed voices' by kind, two per operator of a graph and one per operator whose feedback index
    is a gene (feedback_genes: a mask or a list of operator indices)"""
    if synth_kind == SYNTH_GRAPH:
        if graph is None:
            raise ValueError("SYNTH_GRAPH needs graph=")
        return 2 * int(as_voice_graph(graph).num_operators) + bin(_mask(feedback_genes or 0) & 0xFFFFFFFF).count("1")
    if feedback_genes is not None:  # (also a mask of 0: the caller believes the voice is a graph)
        raise ValueError("feedback_genes needs SYNTH_GRAPH and graph=: a fixed voice has no feedback indices")
    return SYNTH_DIMS[synth_kind]


def _operators(handle):
    """operators of a handle's graph (a view of somebody else's context has only its genes to go by)"""
    g = getattr(handle, "graph", None)
    return handle.D // 2 if g is None else int(g.num_operators)


class Info(C.Structure):
    _fields_ = [
        ("population_length", C.c_uint32), ("num_dimensions", C.c_uint32),
        ("audio_length", C.c_uint32), ("spectrum_row_floats", C.c_uint32),
        ("rotation_index", C.c_uint32), ("generation", C.c_uint32),
        ("compute_units", C.c_uint32), ("reserved", C.c_uint32),
        ("device_name", C.c_char * 128), ("arch", C.c_char * 32),
    ]


class GenRecord(C.Structure):
    """sots_gen_record: one history record of the parent rows (96 bytes)"""
    _fields_ = [
        ("generation", C.c_uint32), ("best_fitness", C.c_float), ("best_ever_fitness", C.c_float),
        ("parent_worst_fitness", C.c_float), ("parent_mean_fitness", C.c_float), ("reserved", C.c_float * 3),
        ("mean_step", C.c_float * MAX_DIMS),
    ]


GEN_RECORD_DTYPE = np.dtype([("generation", np.uint32), ("best_fitness", np.float32), ("best_ever_fitness", np.float32),
                             ("parent_worst_fitness", np.float32), ("parent_mean_fitness", np.float32),
                             ("reserved", np.float32, (3,)), ("mean_step", np.float32, (MAX_DIMS,))])


class StopRule(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("check_interval", C.c_uint32), ("target_fitness", C.c_float),
                ("stall_generations", C.c_uint32)]


class ChunkResult(C.Structure):
    """sots_chunk_result: what the chunk queue stores when it retires a chunk (208 bytes)"""
    _fields_ = [
        ("generations_run", C.c_uint32), ("best_ever_generation", C.c_uint32), ("best_ever_fitness", C.c_float),
        ("last_fitness", C.c_float), ("best_ever_values", C.c_float * MAX_DIMS), ("best_ever_steps", C.c_float * MAX_DIMS),
        ("last_values", C.c_float * MAX_DIMS),
    ]


CHUNK_RESULT_DTYPE = np.dtype([("generations_run", np.uint32), ("best_ever_generation", np.uint32),
                               ("best_ever_fitness", np.float32), ("last_fitness", np.float32),
                               ("best_ever_values", np.float32, (MAX_DIMS,)), ("best_ever_steps", np.float32, (MAX_DIMS,)),
                               ("last_values", np.float32, (MAX_DIMS,))])


class RenderArgs(C.Structure):
    """sots_render_args"""
    _fields_ = [("struct_size", C.c_uint32), ("hop", C.c_uint32), ("flags", C.c_uint32), ("rows_per_pass", C.c_uint32)]


class RenderContinuousArgs(C.Structure):
    """sots_render_continuous_args"""
    _fields_ = [("struct_size", C.c_uint32), ("hop", C.c_uint32), ("flags", C.c_uint32), ("samples_per_pass", C.c_uint32)]


class RenderGraphFeedbackArgs(C.Structure):
    """sots_render_graph_feedback_args"""
    _fields_ = [("struct_size", C.c_uint32), ("hop", C.c_uint32), ("flags", C.c_uint32), ("samples_per_pass", C.c_uint32),
                ("chain_form", C.c_uint32), ("relax_cap", C.c_uint32)]


class QueueStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("slots", C.c_uint32), ("global_generations", C.c_uint64),
                ("chunk_generations", C.c_uint64)]


def make_stop_rule(target=None, stall=0, check_every=32):
    """target None (or negative) = no fitness target; stall 0 = no stall rule"""
    r = StopRule()
    r.struct_size = C.sizeof(StopRule)
    r.check_interval = check_every
    r.target_fitness = -1.0 if target is None else float(target)
    r.stall_generations = stall
    return r


def _track_args(best_ever, history_every, capacity):
    flags = (TRACK_BEST_EVER if best_ever or history_every else 0) | (TRACK_HISTORY if history_every else 0)
    return flags, history_every, capacity if history_every else 0


_lib = None


def load():
    """dlopen libsots_hip.so.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SOTS_LIB_PATH", LIB_PATH)  # development override (kernel variants)
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C <package dir>`; there is no CPU fallback")
    L = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.sots_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.sots_destroy.argtypes = [vp]
    L.sots_destroy.restype = None
    L.sots_last_error.argtypes = [vp]
    L.sots_last_error.restype = C.c_char_p
    L.sots_set_stream.argtypes = [vp, vp]
    L.sots_synchronize.argtypes = [vp]
    L.sots_set_target_audio.argtypes = [vp, vp, u32]
    L.sots_set_target_spectrum.argtypes = [vp, vp, u32]
    L.sots_init_population.argtypes = [vp, u32]
    for name in ("sots_write_population", "sots_read_population", "sots_read_population_other"):
        getattr(L, name).argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.sots_write_synth.argtypes = [vp, vp, sz, vp, sz]
    L.sots_read_synth.argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.sots_set_sort_mode.argtypes = [vp, u32]
    L.sots_set_select_plan.argtypes = [vp, u32]
    L.sots_select_splitter_count.argtypes = [vp, C.POINTER(u32)]
    L.sots_write_select_splitters.argtypes = [vp, vp, u32]
    L.sots_read_select_splitters.argtypes = [vp, vp, u32]
    L.sots_stage_bucket_fitness.argtypes = [vp]
    L.sots_read_select_lists.argtypes = [vp, vp, u32, vp, u32]
    L.sots_set_synth_arithmetic.argtypes = [vp, u32]
    for name in ("recombine", "mutate", "synthesise", "window", "fft", "fitness", "sort", "select", "rotate"):
        getattr(L, "sots_stage_" + name).argtypes = [vp]
    L.sots_execute_generation.argtypes = [vp]
    L.sots_execute_generations.argtypes = [vp, u32]
    L.sots_set_survivors.argtypes = [vp, u32]
    L.sots_get_survivors.argtypes = [vp, C.POINTER(u32)]
    L.sots_set_objective.argtypes = [vp, u32, C.c_float]
    L.sots_get_objective.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float)]
    L.sots_batch_set_objective.argtypes = [vp, u32, C.c_float]
    L.sots_group_set_objective.argtypes = [vp, u32, C.c_float]
    L.sots_set_objective_weights.argtypes = [vp, vp, u32]
    L.sots_get_objective_weights.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.sots_batch_set_objective_weights.argtypes = [vp, vp, u32]
    L.sots_group_set_objective_weights.argtypes = [vp, vp, u32]
    L.sots_get_generation.argtypes = [vp, C.POINTER(u32)]
    L.sots_set_generation.argtypes = [vp, u32]
    L.sots_timing_enable.argtypes = [vp, C.c_int]
    L.sots_timing_reset.argtypes = [vp]
    L.sots_stage_time_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sots_stage_launch_times_ms.argtypes = [vp, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sots_pack_elites_device.argtypes = [vp, vp, u32]
    L.sots_inject_immigrants_device.argtypes = [vp, vp, u32]
    L.sots_inject_gathered_device.argtypes = [vp, vp, u32, u32, u32]
    L.sots_fuse_exchange_next_sort.argtypes = [vp, vp, u32, vp, u32, u32, u32, vp]
    L.sots_pack_elites_host.argtypes = [vp, vp, u32]
    L.sots_inject_immigrants_host.argtypes = [vp, vp, u32]
    L.sots_get_info.argtypes = [vp, C.POINTER(Info)]
    L.sots_group_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int32), u32, u32, u32, u32, C.POINTER(vp)]
    L.sots_group_destroy.argtypes = [vp]
    L.sots_group_destroy.restype = None
    L.sots_group_last_error.argtypes = [vp]
    L.sots_group_last_error.restype = C.c_char_p
    L.sots_group_size.argtypes = [vp]
    L.sots_group_size.restype = u32
    L.sots_group_uses_rccl.argtypes = [vp]
    L.sots_group_island.argtypes = [vp, u32]
    L.sots_group_island.restype = vp
    L.sots_group_set_target_audio.argtypes = [vp, vp, u32]
    L.sots_group_set_target_spectrum.argtypes = [vp, vp, u32]
    L.sots_group_init_population.argtypes = [vp, u32]
    L.sots_group_execute_generations.argtypes = [vp, u32]
    L.sots_group_synchronize.argtypes = [vp]
    L.sots_group_best.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float)]
    L.sots_batch_create.argtypes = [C.POINTER(Config), u32, C.POINTER(vp)]
    L.sots_batch_destroy.argtypes = [vp]
    L.sots_batch_destroy.restype = None
    L.sots_batch_last_error.argtypes = [vp]
    L.sots_batch_last_error.restype = C.c_char_p
    L.sots_batch_synchronize.argtypes = [vp]
    L.sots_batch_set_target_audio.argtypes = [vp, vp, u32, u32]
    L.sots_batch_set_target_spectra.argtypes = [vp, vp, u32, u32]
    L.sots_batch_init_population.argtypes = [vp, u32]
    L.sots_batch_execute_generations.argtypes = [vp, u32]
    L.sots_batch_set_synth_arithmetic.argtypes = [vp, u32]
    L.sots_batch_set_survivors.argtypes = [vp, u32]
    L.sots_batch_read_best.argtypes = [vp, vp, sz, vp, sz]
    L.sots_batch_read_population.argtypes = [vp, u32, vp, sz, vp, sz, vp, sz]
    u64p = C.POINTER(C.c_uint64)
    L.sots_track.argtypes = [vp, u32, u32, u32]
    L.sots_read_best_ever.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_float), C.POINTER(u32)]
    L.sots_read_history.argtypes = [vp, vp, u32, C.POINTER(u32), u64p]
    L.sots_stop_rule_holds.argtypes = [C.POINTER(StopRule), C.c_float, u32, u32]
    L.sots_execute_until.argtypes = [vp, u32, C.POINTER(StopRule), C.POINTER(u32)]
    L.sots_batch_track.argtypes = [vp, u32, u32, u32]
    L.sots_batch_read_best_ever.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz]
    L.sots_batch_read_history.argtypes = [vp, u32, vp, u32, C.POINTER(u32), u64p]
    L.sots_batch_execute_until.argtypes = [vp, u32, C.POINTER(StopRule), C.POINTER(u32)]
    L.sots_batch_queue_targets_spectra.argtypes = [vp, vp, C.c_uint64, u32]
    L.sots_batch_queue_targets_audio.argtypes = [vp, vp, C.c_uint64, u32]
    L.sots_batch_queue_run.argtypes = [vp, u32, u32, C.POINTER(StopRule), u32, C.POINTER(QueueStats)]
    L.sots_batch_queue_results.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.sots_batch_queue_read_kept_population.argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.sots_queue_makespan.argtypes = [C.POINTER(u32), u32, u32, u64p]
    L.sots_render_overlap_add.argtypes = [vp, vp, sz, u32, C.POINTER(RenderArgs), vp, C.c_uint64]
    L.sots_render_continuous.argtypes = [vp, vp, sz, u32, C.POINTER(RenderContinuousArgs), vp, C.c_uint64]
    L.sots_render_graph_continuous.argtypes = [vp, vp, sz, u32, C.POINTER(RenderContinuousArgs), vp, C.c_uint64]
    L.sots_render_graph_feedback.argtypes = [vp, vp, sz, u32, C.POINTER(RenderGraphFeedbackArgs), vp, C.c_uint64]
    L.sots_render_graph_genes.argtypes = [vp, vp, sz, u32, C.POINTER(RenderGraphFeedbackArgs), vp, C.c_uint64]
    L.sots_batch_set_target_audio_hop.argtypes = [vp, vp, u32, u32, u32]
    L.sots_batch_queue_targets_audio_hop.argtypes = [vp, vp, C.c_uint64, u32, u32]
    L.sots_batch_queue_set_carry.argtypes = [vp, u32, u32]
    L.sots_batch_queue_get_carry.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.sots_batch_set_analysis.argtypes = [vp, u32]
    L.sots_batch_get_analysis.argtypes = [vp, C.POINTER(u32)]
    L.sots_batch_analyse_audio_hop.argtypes = [vp, vp, C.c_uint64, u32, u32, vp, C.c_uint64]
    L.sots_batch_queue_score_audio_hop.argtypes = [vp, vp, C.c_uint64, u32, vp, u32]
    L.sots_create_graph.argtypes = [C.POINTER(Config), C.POINTER(VoiceGraph), C.POINTER(vp)]
    L.sots_batch_create_graph.argtypes = [C.POINTER(Config), C.POINTER(VoiceGraph), u32, C.POINTER(vp)]
    L.sots_get_voice_graph.argtypes = [vp, C.POINTER(VoiceGraph)]
    L.sots_set_voice_waveforms.argtypes = [vp, C.POINTER(u32), u32]
    L.sots_get_voice_waveforms.argtypes = [vp, C.POINTER(u32)]
    L.sots_batch_set_voice_waveforms.argtypes = [vp, C.POINTER(u32), u32]
    L.sots_batch_get_voice_waveforms.argtypes = [vp, C.POINTER(u32)]
    L.sots_set_voice_feedback.argtypes = [vp, C.POINTER(C.c_float), u32]
    L.sots_get_voice_feedback.argtypes = [vp, C.POINTER(C.c_float)]
    L.sots_batch_set_voice_feedback.argtypes = [vp, C.POINTER(C.c_float), u32]
    L.sots_batch_get_voice_feedback.argtypes = [vp, C.POINTER(C.c_float)]
    L.sots_create_graph_genes.argtypes = [C.POINTER(Config), C.POINTER(VoiceGraph), u32, C.POINTER(vp)]
    L.sots_batch_create_graph_genes.argtypes = [C.POINTER(Config), C.POINTER(VoiceGraph), u32, u32, C.POINTER(vp)]
    L.sots_get_voice_feedback_genes.argtypes = [vp, C.POINTER(u32)]
    L.sots_batch_get_voice_feedback_genes.argtypes = [vp, C.POINTER(u32)]
    L.sots_set_graph_synth_form.argtypes = [vp, u32]
    L.sots_get_graph_synth_form.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.sots_batch_set_graph_synth_form.argtypes = [vp, u32]
    L.sots_batch_get_graph_synth_form.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.sots_graph_time_parallel_capacity.argtypes = [C.POINTER(VoiceGraph), C.POINTER(u32), C.POINTER(u32)]
    _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _nbytes(a):
    return 0 if a is None else a.nbytes


def make_config(num_parents, num_offspring, synth_kind=SYNTH_2OP, audio_log2=10, param_min=None, param_max=None,
                seed=0x5EED0001, workgroup_size=32, device=0, gid_base=0, num_generations=0, graph=None, feedback_genes=None):
    d = synth_dims(synth_kind, graph, feedback_genes)
    cfg = Config()
    cfg.struct_size = C.sizeof(Config)
    cfg.num_parents, cfg.num_offspring, cfg.num_dimensions = num_parents, num_offspring, d
    cfg.audio_length_log2, cfg.num_generations = audio_log2, num_generations
    cfg.synth_kind, cfg.workgroup_size = synth_kind, workgroup_size
    cfg.device, cfg.gid_base, cfg.seed = device, gid_base, seed
    pmin = list(param_min) if param_min is not None else [0.0] * d
    pmax = list(param_max)
    for i in range(MAX_DIMS):
        cfg.param_min[i] = float(pmin[i]) if i < len(pmin) else 0.0
        cfg.param_max[i] = float(pmax[i]) if i < len(pmax) else 0.0
    return cfg


class HipES:
    """One evolutionary-strategy context on one MI355X (mirror of the C-ABI)."""

    @classmethod
    def borrowed(cls, handle, cfg):
        """A view of a context owned by somebody else (an island of a HipGroup): close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = load()
        self.cfg = cfg
        self.P, self.D, self.N = cfg.num_parents + cfg.num_offspring, cfg.num_dimensions, 1 << cfg.audio_length_log2
        self.num_parents = cfg.num_parents
        self._h = C.c_void_p(handle)
        self._borrowed = True
        return self

    def __init__(self, num_parents, num_offspring, synth_kind=SYNTH_2OP, audio_log2=10,
                 param_min=None, param_max=None, seed=0x5EED0001, workgroup_size=32,
                 device=0, gid_base=0, num_generations=0, graph=None, waveforms=None, feedback=None, feedback_genes=None):
        """graph (with synth_kind=SYNTH_GRAPH): a VoiceGraph or its JSON form, see as_voice_graph; waveforms: that
        graph's operator waveforms, see set_voice_waveforms; feedback: its operators' feedback indices, see
        set_voice_feedback; feedback_genes: the operators whose feedback index is a gene of the individual instead (a
        mask or a list of operator indices, sots_create_graph_genes): D grows by one per operator, and param_min /
        param_max carry those genes' ranges, within [0, 2], behind the 2 OPS others"""
        self.L = load()
        self._borrowed = False
        self.graph = as_voice_graph(graph)
        cfg = make_config(num_parents, num_offspring, synth_kind, audio_log2, param_min, param_max, seed, workgroup_size,
                          device, gid_base, num_generations, graph=self.graph, feedback_genes=feedback_genes)
        self.cfg = cfg
        self.P, self.D, self.N = num_parents + num_offspring, cfg.num_dimensions, 1 << audio_log2
        self.num_parents = num_parents
        h = C.c_void_p()
        if self.graph is not None and feedback_genes is not None:
            rc = self.L.sots_create_graph_genes(C.byref(cfg), C.byref(self.graph), _mask(feedback_genes), C.byref(h))
        elif self.graph is not None:
            rc = self.L.sots_create_graph(C.byref(cfg), C.byref(self.graph), C.byref(h))
        else:
            rc = self.L.sots_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise SotsError(rc, self.L.sots_last_error(None).decode())
        self._h = h
        if waveforms is not None:
            self.set_voice_waveforms(waveforms)
        if feedback is not None:
            self.set_voice_feedback(feedback)

    # -- plumbing --
    def _check(self, rc):
        if rc != 0:
            raise SotsError(rc, self.L.sots_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self.L.sots_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        self._check(self.L.sots_set_stream(self._h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self._check(self.L.sots_synchronize(self._h))

    def voice_graph(self):
        g = VoiceGraph()
        self._check(self.L.sots_get_voice_graph(self._h, C.byref(g)))
        return g

    def set_voice_waveforms(self, waveforms):
        """one WAVE_* code or WAVE_NAMES name per operator of the graph, or None: all sine.  Like a new objective: the run
        record is cleared"""
        codes, count = _waveform_codes(waveforms)
        self._check(self.L.sots_set_voice_waveforms(self._h, codes, count))

    def voice_waveforms(self):
        """the codes of the graph's operators"""
        codes = (C.c_uint32 * GRAPH_MAX_OPERATORS)()
        self._check(self.L.sots_get_voice_waveforms(self._h, codes))
        return list(codes)[:_operators(self)]

    def set_voice_feedback(self, feedback):
        """one feedback index in [0, 2] per operator of the graph, or None: no feedback.  Like set_voice_waveforms: the run
        record is cleared"""
        index, count = _feedback_indices(feedback)
        self._check(self.L.sots_set_voice_feedback(self._h, index, count))

    def voice_feedback(self):
        """the feedback indices of the graph's operators"""
        index = (C.c_float * GRAPH_MAX_OPERATORS)()
        self._check(self.L.sots_get_voice_feedback(self._h, index))
        return list(index)[:_operators(self)]

    def voice_feedback_genes(self):
        """the mask of the operators whose feedback index is a gene (0: none)"""
        mask = C.c_uint32()
        self._check(self.L.sots_get_voice_feedback_genes(self._h, C.byref(mask)))
        return mask.value

    def set_graph_synth_form(self, form):
        """GRAPH_FORM_AUTO (default), GRAPH_FORM_LANES or GRAPH_FORM_TIME_PARALLEL (enum sots_graph_synth_form), or a
        GRAPH_FORM_NAMES name: which synthesis kernel the graph voice runs - the same audio bit for bit either way, and
        nothing is cleared"""
        self._check(self.L.sots_set_graph_synth_form(self._h, GRAPH_FORM_NAMES.get(form, form)))

    def graph_synth_form(self):
        """(requested, effective): effective is what the next synthesis of the handle's own rows would launch"""
        requested, effective = C.c_uint32(), C.c_uint32()
        self._check(self.L.sots_get_graph_synth_form(self._h, C.byref(requested), C.byref(effective)))
        return requested.value, effective.value

    def info(self):
        i = Info()
        self._check(self.L.sots_get_info(self._h, C.byref(i)))
        return i

    # -- target --
    def set_target_audio(self, audio):
        a = _f32(audio)
        self._check(self.L.sots_set_target_audio(self._h, _ptr(a), a.size))

    def set_target_spectrum(self, mag):
        m = _f32(mag)
        self._check(self.L.sots_set_target_spectrum(self._h, _ptr(m), m.size))

    # -- population --
    def init_population(self, chunk=0):
        self._check(self.L.sots_init_population(self._h, chunk))

    def write_population(self, values=None, steps=None, fitness=None):
        v = None if values is None else _f32(values)
        s = None if steps is None else _f32(steps)
        f = None if fitness is None else _f32(fitness)
        self._check(self.L.sots_write_population(self._h, _ptr(v), _nbytes(v), _ptr(s), _nbytes(s),
                                                 _ptr(f), _nbytes(f)))

    def read_population(self, other=False):
        v = np.empty((self.P, self.D), np.float32)
        s = np.empty((self.P, self.D), np.float32)
        f = np.empty(self.P, np.float32)
        fn = self.L.sots_read_population_other if other else self.L.sots_read_population
        self._check(fn(self._h, _ptr(v), v.nbytes, _ptr(s), s.nbytes, _ptr(f), f.nbytes))
        return v, s, f

    def read_fitness(self):
        f = np.empty(self.P, np.float32)
        self._check(self.L.sots_read_population(self._h, None, 0, None, 0, _ptr(f), f.nbytes))
        return f

    # -- synthesiser buffers --
    def write_audio(self, audio):
        a = _f32(audio)
        self._check(self.L.sots_write_synth(self._h, _ptr(a), a.nbytes, None, 0))

    def write_spectrum(self, spectrum):
        s = _f32(spectrum)
        self._check(self.L.sots_write_synth(self._h, None, 0, _ptr(s), s.nbytes))

    def read_audio(self):
        a = np.empty((self.P, self.N), np.float32)
        self._check(self.L.sots_read_synth(self._h, _ptr(a), a.nbytes, None, 0, None, 0))
        return a

    def read_spectrum(self):
        """complex64 [P][N/2+4]; bins 0..N/2 valid."""
        s = np.empty((self.P, self.N + 8), np.float32)
        self._check(self.L.sots_read_synth(self._h, None, 0, _ptr(s), s.nbytes, None, 0))
        return s.view(np.complex64)

    def read_target(self):
        t = np.empty(self.N // 2, np.float32)
        self._check(self.L.sots_read_synth(self._h, None, 0, None, 0, _ptr(t), t.nbytes))
        return t

    # -- rendering of a parameter track: the rows, the output and the call that the four renderers share --
    def _render(self, entry, values, hop, out_samples, args):
        v = _f32(values).reshape(-1, self.D)
        rows = v.shape[0]
        n_out = (rows - 1) * hop + self.N if out_samples is None else int(out_samples)
        out = np.empty(max(n_out, 0), np.float32)
        self._check(entry(self._h, _ptr(v), v.nbytes, rows, C.byref(args), _ptr(out), out.size))
        return out

    # -- overlap-add rendering of a parameter track --
    def render_overlap_add(self, values, hop, windowed=True, rows_per_pass=0, out_samples=None):
        """values[M][D] unit-range genes, row c standing for samples [c hop, c hop + N): the windowed (or rectangular)
        overlap-add of the rows' audio, normalised by the summed window.  out_samples None: the covered (M-1) hop + N."""
        args = RenderArgs(C.sizeof(RenderArgs), hop, RENDER_WINDOWED if windowed else 0, rows_per_pass)
        return self._render(self.L.sots_render_overlap_add, values, hop, out_samples, args)

    # -- phase-continuous rendering of a parameter track --
    def render_continuous(self, values, hop, glide=False, samples_per_pass=0, out_samples=None):
        """values[M][D] unit-range genes, row c anchored at sample c hop + N/2: the track as one voice whose oscillators
        never restart, the genes held from anchor to anchor (switching half way) or, with glide, interpolated between
        them.  out_samples None: (M-1) hop + N."""
        args = RenderContinuousArgs(C.sizeof(RenderContinuousArgs), hop, RENDER_GLIDE if glide else 0, samples_per_pass)
        return self._render(self.L.sots_render_continuous, values, hop, out_samples, args)

    # -- phase-continuous rendering of a parameter track of the operator-graph voice --
    def render_graph_continuous(self, values, hop, glide=False, samples_per_pass=0, out_samples=None):
        """render_continuous for a context of the graph voice (graph=...), with its waveforms: values[M][2 x operators].
        A context with a feedback index other than 0 is refused (render_overlap_add renders it)."""
        args = RenderContinuousArgs(C.sizeof(RenderContinuousArgs), hop, RENDER_GLIDE if glide else 0, samples_per_pass)
        return self._render(self.L.sots_render_graph_continuous, values, hop, out_samples, args)

    # -- ... with feedback operators --
    def render_graph_feedback(self, values, hop, glide=False, samples_per_pass=0, chain_form=0, relax_cap=0, out_samples=None):
        """render_graph_continuous for a context whose operators may have feedback indices (set_voice_feedback).
        chain_form: CHAIN_LIBRARY, CHAIN_SERIAL or CHAIN_RELAX; relax_cap: sweeps per tile before a tile is finished serially
        (0: the library's choice).  Neither changes a bit of the result."""
        args = RenderGraphFeedbackArgs(C.sizeof(RenderGraphFeedbackArgs), hop, RENDER_GLIDE if glide else 0, samples_per_pass, chain_form, relax_cap)
        return self._render(self.L.sots_render_graph_feedback, values, hop, out_samples, args)

    # -- ... whose feedback indices are genes --
    def render_graph_genes(self, values, hop, glide=False, samples_per_pass=0, chain_form=0, relax_cap=0, out_samples=None):
        """render_graph_feedback for a context of feedback_genes=...: values[M][2 x operators + E], every row with its own
        indices, held or glided like every gene.  With a mask of 0 it is render_graph_feedback."""
        args = RenderGraphFeedbackArgs(C.sizeof(RenderGraphFeedbackArgs), hop, RENDER_GLIDE if glide else 0, samples_per_pass, chain_form, relax_cap)
        return self._render(self.L.sots_render_graph_genes, values, hop, out_samples, args)

    # -- stages --
    def recombine(self):
        self._check(self.L.sots_stage_recombine(self._h))

    def mutate(self):
        self._check(self.L.sots_stage_mutate(self._h))

    def synthesise(self):
        self._check(self.L.sots_stage_synthesise(self._h))

    def window(self):
        self._check(self.L.sots_stage_window(self._h))

    def fft(self):
        self._check(self.L.sots_stage_fft(self._h))

    def fitness(self):
        self._check(self.L.sots_stage_fitness(self._h))

    def sort(self):
        self._check(self.L.sots_stage_sort(self._h))

    def select(self):
        self._check(self.L.sots_stage_select(self._h))

    def bucket_fitness(self):
        """files the current half's keys between the splitters the next select() reads: that select() takes list mode"""
        self._check(self.L.sots_stage_bucket_fitness(self._h))

    def read_select_lists(self):
        """what bucket_fitness() filed: counts[B, 16] (every key of a closed bucket, per segment) and keys[B, 16, 128]"""
        b = self.select_splitter_count()
        counts, keys = np.empty((b, 16), np.uint32), np.empty((b, 16, 128), np.uint64)
        self._check(self.L.sots_read_select_lists(self._h, counts.ctypes.data_as(C.c_void_p), counts.size, keys.ctypes.data_as(C.c_void_p), keys.size))
        return counts, keys

    def rotate(self):
        self._check(self.L.sots_stage_rotate(self._h))

    def set_sort_mode(self, mode):
        self._check(self.L.sots_set_sort_mode(self._h, mode))

    def set_select_plan(self, plan):
        """SELECT_AUTO (default), SELECT_TILES or SELECT_SPLITTERS (enum sots_select_plan): the same rows either way"""
        self._check(self.L.sots_set_select_plan(self._h, plan))

    def select_splitter_count(self):
        n = C.c_uint32()
        self._check(self.L.sots_select_splitter_count(self._h, C.byref(n)))
        return n.value

    def write_select_splitters(self, keys):
        """the 64-bit keys the next SPLITTERS selection ranks between (any values give the exact rows)"""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        self._check(self.L.sots_write_select_splitters(self._h, k.ctypes.data_as(C.c_void_p), k.size))

    def read_select_splitters(self):
        k = np.empty(self.select_splitter_count(), np.uint64)
        self._check(self.L.sots_read_select_splitters(self._h, k.ctypes.data_as(C.c_void_p), k.size))
        return k

    def set_synth_arithmetic(self, arith):
        """ARITH_CPU_PATH (default) or ARITH_DEVICE_KERNELS: the reference's OpenCL kernels' arithmetic (enum sots_synth_arith)"""
        self._check(self.L.sots_set_synth_arithmetic(self._h, arith))

    def set_survivors(self, n):
        """rows 0..n-1 of the sorted half pass through variation unchanged (0 <= n <= numParents; 0, the default, is the
        reference's non-elitist strategy); a setting: init_population and set_target_* keep it"""
        self._check(self.L.sots_set_survivors(self._h, n))

    @property
    def survivors(self):
        n = C.c_uint32()
        self._check(self.L.sots_get_survivors(self._h, C.byref(n)))
        return n.value

    def set_objective(self, objective, floor=0.0):
        """OBJECTIVE_MAGNITUDE (default: sum (m - t)^2, the reference's) or OBJECTIVE_LOG_MAGNITUDE: sum (ln(m + floor) -
        ln(t + floor))^2 with 1e-30 <= floor <= 1 in the unit of the normalised magnitudes.  Acts like a new target (the
        run record starts over); before or after set_target_*, with the same result.  Fitness, history and stop-rule
        thresholds are in the units of the active objective."""
        self._check(self.L.sots_set_objective(self._h, objective, floor))

    @property
    def objective(self):
        """(objective, floor); the floor reads 0 under OBJECTIVE_MAGNITUDE"""
        o, f = C.c_uint32(), C.c_float()
        self._check(self.L.sots_get_objective(self._h, C.byref(o), C.byref(f)))
        return o.value, f.value

    def set_objective_weights(self, weights):
        """Per-bin weights w[N/2] of the objective, F = sum_k w_k e_k^2 with e_k the active objective's signed error of bin k
        (finite, >= 0, not all zero), or None for none (the default).  Acts like a new target; before or after
        set_target_* and set_objective, with the same result.  Fitness, history and stop-rule thresholds are in the units
        of the weighted sum."""
        if weights is None:
            self._check(self.L.sots_set_objective_weights(self._h, None, 0))
            return
        w = _f32(weights)
        self._check(self.L.sots_set_objective_weights(self._h, _ptr(w), w.size))

    def get_objective_weights(self):
        """the weights as they were set, or None"""
        is_set = C.c_uint32()
        w = np.empty(self.N // 2, np.float32)
        self._check(self.L.sots_get_objective_weights(self._h, _ptr(w), w.size, C.byref(is_set)))
        return w if is_set.value else None

    def execute_generation(self):
        self._check(self.L.sots_execute_generation(self._h))

    def execute_generations(self, n):
        self._check(self.L.sots_execute_generations(self._h, n))

    @property
    def generation(self):
        g = C.c_uint32()
        self._check(self.L.sots_get_generation(self._h, C.byref(g)))
        return g.value

    @generation.setter
    def generation(self, g):
        self._check(self.L.sots_set_generation(self._h, g))

    # -- run record: best-ever individual, history, stop rules --
    def track(self, best_ever=True, history_every=0, capacity=1024):
        """best-ever record and, with history_every > 0, a ring of the newest `capacity` per-generation records;
        track(False) switches it off.  Any call starts from cleared records."""
        self._check(self.L.sots_track(self._h, *_track_args(best_ever, history_every, capacity)))
        self._history_capacity = capacity if history_every else 0

    def best_ever(self):
        """(values[D], steps[D], fitness, generation) of the best individual seen since the last clear"""
        v = np.empty(self.D, np.float32)
        s = np.empty(self.D, np.float32)
        f, g = C.c_float(), C.c_uint32()
        self._check(self.L.sots_read_best_ever(self._h, _ptr(v), v.nbytes, _ptr(s), s.nbytes, C.byref(f), C.byref(g)))
        return v, s, np.float32(f.value), g.value

    def history(self, with_taken=False):
        """the records held, oldest first, as a structured array (GEN_RECORD_DTYPE)"""
        out = np.zeros(max(1, getattr(self, "_history_capacity", 0)), GEN_RECORD_DTYPE)
        n, taken = C.c_uint32(), C.c_uint64()
        self._check(self.L.sots_read_history(self._h, _ptr(out), out.size, C.byref(n), C.byref(taken)))
        return (out[:n.value].copy(), taken.value) if with_taken else out[:n.value].copy()

    def execute_until(self, max_generations, target=None, stall=0, check_every=32):
        """generations in blocks of check_every until the best-ever fitness is <= target or has not improved for
        `stall` generations; returns the generations run"""
        rule = make_stop_rule(target, stall, check_every)
        run = C.c_uint32()
        self._check(self.L.sots_execute_until(self._h, max_generations, C.byref(rule), C.byref(run)))
        return run.value

    # -- timing --
    def timing_enable(self, on=True):
        self._check(self.L.sots_timing_enable(self._h, 1 if on else 0))

    def timing_reset(self):
        self._check(self.L.sots_timing_reset(self._h))

    def stage_time_ms(self, stage):
        t, c = C.c_double(), C.c_uint64()
        self._check(self.L.sots_stage_time_ms(self._h, stage, C.byref(t), C.byref(c)))
        return t.value, c.value

    def stage_launch_times_ms(self, stage, capacity=65536):
        out = np.empty(capacity, np.float32)
        n = C.c_uint64()
        self._check(self.L.sots_stage_launch_times_ms(self._h, stage, _ptr(out), capacity, C.byref(n)))
        return out[:n.value].copy()

    # -- island exchange --
    def pack_elites_device(self, dev_ptr, n_rows):
        self._check(self.L.sots_pack_elites_device(self._h, C.c_void_p(dev_ptr), n_rows))

    def inject_immigrants_device(self, dev_ptr, n_rows):
        self._check(self.L.sots_inject_immigrants_device(self._h, C.c_void_p(dev_ptr), n_rows))

    def inject_gathered_device(self, dev_ptr, world, rank, elites):
        self._check(self.L.sots_inject_gathered_device(self._h, C.c_void_p(dev_ptr), world, rank, elites))

    def sort_places(self, n_rows):
        """True when every generation's sortPopulation places at least the first n_rows rows (the selection places
        rows 0..S-1 only, S = the whole parent blocks and never fewer than the parents; enum sots_sort_mode)."""
        block = max(1, self.cfg.workgroup_size)
        breeding = max(1, self.cfg.num_parents // block) * block
        return n_rows <= max(breeding, self.cfg.num_parents)

    def fuse_exchange_next_sort(self, elite_ptr, n_elite_rows, gathered_ptr, world, rank, elites, host_gate_event=None):
        """pack + inject folded into the sort of the last generation of the next execute_generations call; the host
        waits for host_gate_event (a raw hipEvent_t) right before it enqueues that sort"""
        self._check(self.L.sots_fuse_exchange_next_sort(self._h, C.c_void_p(elite_ptr) if elite_ptr else None, n_elite_rows,
                                                        C.c_void_p(gathered_ptr) if gathered_ptr else None, world, rank, elites,
                                                        C.c_void_p(host_gate_event) if host_gate_event else None))

    def pack_elites(self, n_rows):
        rows = np.empty((n_rows, 2 * self.D + 1), np.float32)
        self._check(self.L.sots_pack_elites_host(self._h, _ptr(rows), n_rows))
        return rows

    def inject_immigrants(self, rows):
        r = _f32(rows)
        self._check(self.L.sots_inject_immigrants_host(self._h, _ptr(r), r.shape[0]))


class HipBatch:
    """Chunks in flight (sots_batch_* of the C-ABI): up to max_chunks independent populations of one shape, each against
    its own target, advanced by the launches of one population per generation.  Chunk c computes bit for bit what a
    HipES of the same arguments computes after init_population(first + c)."""

    def __init__(self, max_chunks, num_parents, num_offspring, synth_kind=SYNTH_2OP, audio_log2=10, param_min=None,
                 param_max=None, seed=0x5EED0001, workgroup_size=32, device=0, gid_base=0, num_generations=0, graph=None,
                 waveforms=None, feedback=None, feedback_genes=None):
        """feedback_genes: as for HipES (sots_batch_create_graph_genes)"""
        self.L = load()
        self.graph = as_voice_graph(graph)
        self.cfg = make_config(num_parents, num_offspring, synth_kind, audio_log2, param_min, param_max, seed, workgroup_size,
                               device, gid_base, num_generations, graph=self.graph, feedback_genes=feedback_genes)
        self.P, self.D, self.N = num_parents + num_offspring, self.cfg.num_dimensions, 1 << audio_log2
        self.max_chunks = max_chunks
        self.active = 0
        self.queued = 0
        h = C.c_void_p()
        if self.graph is not None and feedback_genes is not None:
            rc = self.L.sots_batch_create_graph_genes(C.byref(self.cfg), C.byref(self.graph), _mask(feedback_genes), max_chunks, C.byref(h))
        elif self.graph is not None:
            rc = self.L.sots_batch_create_graph(C.byref(self.cfg), C.byref(self.graph), max_chunks, C.byref(h))
        else:
            rc = self.L.sots_batch_create(C.byref(self.cfg), max_chunks, C.byref(h))
        if rc != 0:
            raise SotsError(rc, self.L.sots_batch_last_error(None).decode())
        self._h = h
        if waveforms is not None:
            self.set_voice_waveforms(waveforms)
        if feedback is not None:
            self.set_voice_feedback(feedback)

    def _check(self, rc):
        if rc != 0:
            raise SotsError(rc, self.L.sots_batch_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.L.sots_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.L.sots_batch_synchronize(self._h))

    def set_target_audio(self, audio, hop=None):
        """audio[num_chunks][N] (or a flat signal cut into N-sample chunks): one target per chunk.  With hop, a flat
        signal whose chunk k is samples [k hop, k hop + N)."""
        a = _f32(audio)
        if hop is not None:
            a = a.reshape(-1)
            chunks = (a.size - self.N) // hop + 1 if a.size >= self.N and hop > 0 else 0
            self._check(self.L.sots_batch_set_target_audio_hop(self._h, _ptr(a), a.size, hop, chunks))
            self.active = chunks
            return
        chunks = a.shape[0] if a.ndim == 2 else a.size // self.N
        self._check(self.L.sots_batch_set_target_audio(self._h, _ptr(a), a.size, chunks))
        self.active = chunks

    def set_target_spectra(self, mags):
        """mags[num_chunks][N/2]"""
        m = _f32(mags)
        chunks = m.shape[0] if m.ndim == 2 else m.size // (self.N // 2)
        self._check(self.L.sots_batch_set_target_spectra(self._h, _ptr(m), m.size, chunks))
        self.active = chunks

    def init_population(self, first=0):
        self._check(self.L.sots_batch_init_population(self._h, first))

    def execute_generations(self, n):
        self._check(self.L.sots_batch_execute_generations(self._h, n))

    def set_synth_arithmetic(self, arith):
        self._check(self.L.sots_batch_set_synth_arithmetic(self._h, arith))

    def set_survivors(self, n):
        """HipES.set_survivors for every chunk, in execute_generations / execute_until and queue_run alike"""
        self._check(self.L.sots_batch_set_survivors(self._h, n))

    def set_objective(self, objective, floor=0.0):
        """HipES.set_objective for every chunk, in execute_generations / execute_until and queue_run alike"""
        self._check(self.L.sots_batch_set_objective(self._h, objective, floor))

    def set_objective_weights(self, weights):
        """HipES.set_objective_weights for every chunk (one table), in execute_generations / execute_until and queue_run alike"""
        if weights is None:
            self._check(self.L.sots_batch_set_objective_weights(self._h, None, 0))
            return
        w = _f32(weights)
        self._check(self.L.sots_batch_set_objective_weights(self._h, _ptr(w), w.size))

    def set_voice_waveforms(self, waveforms):
        """HipES.set_voice_waveforms for every chunk (one setting), in execute_generations / execute_until and queue_run alike"""
        codes, count = _waveform_codes(waveforms)
        self._check(self.L.sots_batch_set_voice_waveforms(self._h, codes, count))

    def voice_waveforms(self):
        codes = (C.c_uint32 * GRAPH_MAX_OPERATORS)()
        self._check(self.L.sots_batch_get_voice_waveforms(self._h, codes))
        return list(codes)[:_operators(self)]

    def set_voice_feedback(self, feedback):
        """HipES.set_voice_feedback for every chunk (one setting), in execute_generations / execute_until and queue_run alike"""
        index, count = _feedback_indices(feedback)
        self._check(self.L.sots_batch_set_voice_feedback(self._h, index, count))

    def voice_feedback(self):
        index = (C.c_float * GRAPH_MAX_OPERATORS)()
        self._check(self.L.sots_batch_get_voice_feedback(self._h, index))
        return list(index)[:_operators(self)]

    def voice_feedback_genes(self):
        mask = C.c_uint32()
        self._check(self.L.sots_batch_get_voice_feedback_genes(self._h, C.byref(mask)))
        return mask.value

    def set_graph_synth_form(self, form):
        """GRAPH_FORM_AUTO (default), GRAPH_FORM_LANES or GRAPH_FORM_TIME_PARALLEL (enum sots_graph_synth_form), or a
        GRAPH_FORM_NAMES name: which synthesis kernel the graph voice runs - the same audio bit for bit either way, and
        nothing is cleared"""
        self._check(self.L.sots_batch_set_graph_synth_form(self._h, GRAPH_FORM_NAMES.get(form, form)))

    def graph_synth_form(self):
        """(requested, effective): effective is what the next synthesis of the handle's own rows would launch"""
        requested, effective = C.c_uint32(), C.c_uint32()
        self._check(self.L.sots_batch_get_graph_synth_form(self._h, C.byref(requested), C.byref(effective)))
        return requested.value, effective.value

    def read_best(self):
        """(values[active][D], fitness[active]): row 0 of every active chunk"""
        v = np.empty((self.active, self.D), np.float32)
        f = np.empty(self.active, np.float32)
        self._check(self.L.sots_batch_read_best(self._h, _ptr(v), v.nbytes, _ptr(f), f.nbytes))
        return v, f

    def read_population(self, chunk):
        v = np.empty((self.P, self.D), np.float32)
        s = np.empty((self.P, self.D), np.float32)
        f = np.empty(self.P, np.float32)
        self._check(self.L.sots_batch_read_population(self._h, chunk, _ptr(v), v.nbytes, _ptr(s), s.nbytes, _ptr(f), f.nbytes))
        return v, s, f

    # -- run record, per chunk (as HipES) --
    def track(self, best_ever=True, history_every=0, capacity=1024):
        self._check(self.L.sots_batch_track(self._h, *_track_args(best_ever, history_every, capacity)))
        self._history_capacity = capacity if history_every else 0

    def best_ever(self):
        """(values[active][D], steps[active][D], fitness[active], generation[active])"""
        v = np.empty((self.active, self.D), np.float32)
        s = np.empty((self.active, self.D), np.float32)
        f = np.empty(self.active, np.float32)
        g = np.empty(self.active, np.uint32)
        self._check(self.L.sots_batch_read_best_ever(self._h, _ptr(v), v.nbytes, _ptr(s), s.nbytes, _ptr(f), f.nbytes, _ptr(g), g.nbytes))
        return v, s, f, g

    def history(self, chunk, with_taken=False):
        out = np.zeros(max(1, getattr(self, "_history_capacity", 0)), GEN_RECORD_DTYPE)
        n, taken = C.c_uint32(), C.c_uint64()
        self._check(self.L.sots_batch_read_history(self._h, chunk, _ptr(out), out.size, C.byref(n), C.byref(taken)))
        return (out[:n.value].copy(), taken.value) if with_taken else out[:n.value].copy()

    def execute_until(self, max_generations, target=None, stall=0, check_every=32):
        """stops at the first boundary at which the rule holds for every active chunk; returns the generations run"""
        rule = make_stop_rule(target, stall, check_every)
        run = C.c_uint32()
        self._check(self.L.sots_batch_execute_until(self._h, max_generations, C.byref(rule), C.byref(run)))
        return run.value

    # -- chunk queue: any number of chunks through the handle's slots, a slot refilled when its chunk's rule holds --
    def queue_targets_audio(self, audio, hop=None):
        """audio[M][N] (or a flat signal cut into N-sample chunks): the targets of M queued chunks, any M.  With hop, a
        flat signal whose chunk k is samples [k hop, k hop + N)."""
        a = _f32(audio)
        if hop is not None:
            a = a.reshape(-1)
            chunks = (a.size - self.N) // hop + 1 if a.size >= self.N and hop > 0 else 0
            self._check(self.L.sots_batch_queue_targets_audio_hop(self._h, _ptr(a), a.size, hop, chunks))
            self.queued = chunks
            return
        chunks = a.shape[0] if a.ndim == 2 else a.size // self.N
        self._check(self.L.sots_batch_queue_targets_audio(self._h, _ptr(a), a.size, chunks))
        self.queued = chunks

    def queue_targets_spectra(self, mags):
        """mags[M][N/2]"""
        m = _f32(mags)
        chunks = m.shape[0] if m.ndim == 2 else m.size // (self.N // 2)
        self._check(self.L.sots_batch_queue_targets_spectra(self._h, _ptr(m), m.size, chunks))
        self.queued = chunks

    def queue_run(self, first, max_generations, target=None, stall=0, check_every=32, keep=None):
        """every queued chunk until ITS rule holds (no target and no stall: max_generations each, rule = NULL); returns
        (results, stats): a structured array (CHUNK_RESULT_DTYPE), chunk 0 first, and {slots, global_generations,
        chunk_generations}.  keep: a chunk whose whole population is kept for queue_kept_population()."""
        no_rule = (target is None or target < 0) and not stall
        rule = None if no_rule else C.byref(make_stop_rule(target, stall, check_every))
        stats = QueueStats()
        stats.struct_size = C.sizeof(QueueStats)
        self._check(self.L.sots_batch_queue_run(self._h, first, max_generations, rule, QUEUE_NO_CHUNK if keep is None else keep,
                                                C.byref(stats)))
        self.active = 0  # the ordinary calls need set_target_* again
        out = np.zeros(self.queued, CHUNK_RESULT_DTYPE)
        n = C.c_uint32()
        self._check(self.L.sots_batch_queue_results(self._h, _ptr(out), out.size, C.byref(n)))
        return out[:n.value], {"slots": stats.slots, "global_generations": stats.global_generations,
                               "chunk_generations": stats.chunk_generations}

    def queue_set_carry(self, carry_rows, segment_chunks=0):
        """queue_run only: the queued chunks are cut into segments of segment_chunks, and inside a segment a chunk starts
        from its predecessor's best-ever record (row 0) and rows 1..carry_rows-1, beside fresh rows.  carry_rows 0: off.
        Use it with set_survivors(>= 1)."""
        self._check(self.L.sots_batch_queue_set_carry(self._h, carry_rows, segment_chunks))

    def queue_carry(self):
        """(carry_rows, segment_chunks); (0, 0) when off"""
        r, l = C.c_uint32(), C.c_uint32()
        self._check(self.L.sots_batch_queue_get_carry(self._h, C.byref(r), C.byref(l)))
        return r.value, l.value

    # -- analysis on the device --
    def set_analysis(self, mode):
        """ANALYSIS_HOST (the default) or ANALYSIS_DEVICE: how set_target_audio / queue_targets_audio make their spectra.
        The device's fp32 magnitudes are not the host's fp64 bits: a run against one does not repeat a run against the other."""
        self._check(self.L.sots_batch_set_analysis(self._h, mode))

    def get_analysis(self):
        m = C.c_uint32()
        self._check(self.L.sots_batch_get_analysis(self._h, C.byref(m)))
        return m.value

    def _frames(self, a, hop, frames):
        if frames is not None:
            return frames
        return (a.size - self.N) // hop + 1 if a.size >= self.N and hop > 0 else 0

    def analyse_audio_hop(self, audio, hop, frames=None):
        """magnitudes[frames][N/2] of a flat signal's frames [k hop, k hop + N), made on the device whatever the mode;
        frames None: as many as the signal holds"""
        a = _f32(audio).reshape(-1)
        frames = self._frames(a, hop, frames)
        out = np.empty((frames, self.N // 2), np.float32)
        self._check(self.L.sots_batch_analyse_audio_hop(self._h, _ptr(a), a.size, hop, frames, _ptr(out), out.size))
        return out

    def queue_score_audio_hop(self, audio, hop, chunks=None):
        """fitness[chunks]: frame k of a flat signal against stored queue target k under the batch's objective and weights"""
        a = _f32(audio).reshape(-1)
        chunks = self._frames(a, hop, chunks)
        out = np.empty(chunks, np.float32)
        self._check(self.L.sots_batch_queue_score_audio_hop(self._h, _ptr(a), a.size, hop, _ptr(out), chunks))
        return out

    def queue_kept_population(self):
        v = np.empty((self.P, self.D), np.float32)
        s = np.empty((self.P, self.D), np.float32)
        f = np.empty(self.P, np.float32)
        self._check(self.L.sots_batch_queue_read_kept_population(self._h, _ptr(v), v.nbytes, _ptr(s), s.nbytes, _ptr(f), f.nbytes))
        return v, s, f

    @staticmethod
    def queue_makespan(generations_run, slots):
        """the global generations an in-order refill of `slots` slots takes for these per-chunk counts (host only)"""
        g = np.ascontiguousarray(generations_run, dtype=np.uint32)
        out = C.c_uint64()
        rc = load().sots_queue_makespan(g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size, slots, C.byref(out))
        if rc != 0:
            raise SotsError(rc, "sots_queue_makespan: slots must be at least 1")
        return out.value


class HipGroup:
    """Islands inside the library: one process, one island per listed device (sots_group_* of the C-ABI)."""

    def __init__(self, devices, num_elites, num_parents, num_offspring, synth_kind=SYNTH_2OP, audio_log2=10,
                 param_min=None, param_max=None, seed=0x5EED0001, workgroup_size=32, gid_base=0,
                 migration_interval=1, overlap=False, force_rccl=False, unfused=False, event_waits=False):
        self.L = load()
        self.cfg = make_config(num_parents, num_offspring, synth_kind, audio_log2, param_min, param_max, seed, workgroup_size,
                               0, gid_base)
        devs = (C.c_int32 * len(devices))(*devices)
        flags = (GROUP_OVERLAP if overlap else 0) | (GROUP_FORCE_RCCL if force_rccl else 0) | (GROUP_UNFUSED if unfused else 0) | (GROUP_EVENT_WAITS if event_waits else 0)
        h = C.c_void_p()
        rc = self.L.sots_group_create(C.byref(self.cfg), devs, len(devices), num_elites, migration_interval, flags, C.byref(h))
        if rc != 0:
            raise SotsError(rc, self.L.sots_group_last_error(None).decode())
        self._h = h
        self.size = self.L.sots_group_size(h)
        self.uses_rccl = bool(self.L.sots_group_uses_rccl(h))

    def _check(self, rc):
        if rc != 0:
            raise SotsError(rc, self.L.sots_group_last_error(self._h).decode())

    def island(self, i):
        h = self.L.sots_group_island(self._h, i)
        if not h:
            raise IndexError(i)
        return HipES.borrowed(h, self.cfg)

    def set_target_audio(self, audio):
        a = _f32(audio)
        self._check(self.L.sots_group_set_target_audio(self._h, _ptr(a), a.size))

    def set_objective(self, objective, floor=0.0):
        """HipES.set_objective on every island"""
        self._check(self.L.sots_group_set_objective(self._h, objective, floor))

    def set_objective_weights(self, weights):
        """HipES.set_objective_weights on every island"""
        if weights is None:
            self._check(self.L.sots_group_set_objective_weights(self._h, None, 0))
            return
        w = _f32(weights)
        self._check(self.L.sots_group_set_objective_weights(self._h, _ptr(w), w.size))

    def init_population(self, chunk=0):
        self._check(self.L.sots_group_init_population(self._h, chunk))

    def execute_generations(self, n):
        self._check(self.L.sots_group_execute_generations(self._h, n))

    def synchronize(self):
        self._check(self.L.sots_group_synchronize(self._h))

    def best(self):
        i, f = C.c_uint32(), C.c_float()
        self._check(self.L.sots_group_best(self._h, C.byref(i), C.byref(f)))
        return i.value, f.value

    def close(self):
        if getattr(self, "_h", None):
            self.L.sots_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Seeded sequences of C-ABI calls, the facts that make them legal, and their plainest replay.  Pure Python and NumPy.

A seed yields one list of operations for the SUBJECT context (A).  The REFERENCE (B) is a fresh context that runs the
normalised list: the same logical history by the plainest path the library has - SORT_FULL and SELECT_TILES throughout,
every generation a single execute_generation(), no read between checkpoints, no selection setting, no rendering, no
refused call.  A == B at every checkpoint says that nothing the context keeps between calls (pending tails, splitter
slots, key lists, derived target tables, the run record, the occupancy cache) leaks into results.

An operation is a tuple (name, args...) of plain Python values; arrays are named by small integers and made by the
functions at the end of this file, so a list prints as Python that can be pasted (op_text).

The legality rules, each with the sentence of include/sots_hip.h that decides it:
  * "rows S..P-1 are never produced (their content is unspecified ...)" (SOTS_SORT_TOP_ONLY): while a selection's rest
    is outstanding under TOP_ONLY no stage that reads those rows and no partial write_population is emitted, and a
    checkpoint compares rows 0..S-1.
  * "Calls that WRITE rows (stages, write_population, init) end the pending state": after one of them under TOP_ONLY the
    rest can no longer be produced; leaving the mode then completes nothing (situation e).
  * "The next generation's recombinePopulation reads whole parent blocks only": a generation, fused or staged, and a
    stage group that starts at recombine are legal whatever rows S..P-1 hold, and define every row afterwards.
  * sots_execute_generations: "afterwards the audio buffer holds the UN-windowed synthesis and the spectrum buffer is
    untouched": B runs the staged loop, so a stage group never starts at window, fft or fitness - it starts at recombine,
    at synthesise or at sort.
  * sots_stage_select "must be followed by sots_stage_rotate": bucket_fitness .. select, rotate is one unit.
  * sots_track: "the single sots_stage_* calls do not [record]": stage groups are mirrored on B as the same stage calls.
"""
import numpy as np

SORT_LAZY, SORT_FULL, SORT_TOP = 0, 1, 2
PLAN_AUTO, PLAN_TILES, PLAN_SPLITTERS = 0, 1, 2
MAGNITUDE, LOG = 0, 1
SYNTH_2OP, SYNTH_3OP, SYNTH_GRAPH = 0, 1, 4
EDGE_GENERATIONS = (0xFFFFFFFF, 0x80000000)  # tests/_variation_model.py: a Philox counter word about to wrap, its top bit
CHAIN3 = (3, [0, 0b1, 0b10], 0b100)          # tests/_graph_voice_model.py GRAPHS["chain3"]

SHAPES = {
    # P >= 3072 at N = 1024: the wide spectral kernel files keys in the fused loop; 1024 < P: lazy tail, both plans
    "lists": dict(kind=SYNTH_2OP, log2n=10, parents=1024, offspring=3072, block=32, pmax=[3520.0, 8.0, 3520.0, 1.0]),
    # N = 2048: the long rows' tables rebuilt by every target and objective; selection without lists in the loop
    "long": dict(kind=SYNTH_3OP, log2n=11, parents=512, offspring=1536, block=32, pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]),
    # one-launch sort, no selection: every selection setting must be inert
    "small": dict(kind=SYNTH_2OP, log2n=8, parents=64, offspring=192, block=32, pmax=[3520.0, 8.0, 3520.0, 1.0]),
    # chain3 with operator 2's feedback index a gene: D = 7, the voice setters
    "graph": dict(kind=SYNTH_GRAPH, log2n=8, parents=1024, offspring=3072, block=32, graph=CHAIN3, feedback_genes=0b100,
                  pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0, 2.0]),
}
SEEDS = {name: [3200 + 100 * i + j for j in range(12)] for i, name in enumerate(SHAPES)}
OPS = 60

SITUATIONS = {
    "a": "a read while a lazy tail is pending",
    "b": "init_population while a tail is pending",
    "c": "write_population while a tail is pending",
    "d": "leaving TOP_ONLY with the unsorted half intact",
    "e": "leaving TOP_ONLY after it was overwritten",
    "f": "a landscape setter between two execute_generations with no read between",
    "g": "a plan switch between two execute_generations",
    "h": "write_select_splitters followed by a fused generation",
    "i": "bucket_fitness whose lists are then invalidated before select",
    "j": "a refused call between two generations",
    "k": "a rendering between two generations",
    "l": "tracking switched on, off and on again with generations between",
    "m": "a history ring that wraps",
    "n": "the same setter value set twice",
    "o": "LOG floor changed while LOG is active",
    "p": "a refused write_population while a rest is outstanding under TOP_ONLY",
}
# what cannot occur on a shape: without a selection there is no tail, and plans, splitters and lists are inert
IMPOSSIBLE = {"lists": "", "long": "", "graph": "", "small": "abcdeghip"}


class Shape:
    def __init__(self, name):
        c = SHAPES[name]
        self.name, self.kind, self.log2n = name, c["kind"], c["log2n"]
        self.parents, self.offspring, self.block = c["parents"], c["offspring"], c["block"]
        self.pmax, self.graph, self.feedback_genes = c["pmax"], c.get("graph"), c.get("feedback_genes")
        self.N, self.P, self.D = 1 << self.log2n, self.parents + self.offspring, len(c["pmax"])
        self.breeding = max(1, self.parents // self.block) * self.block   # sots_rules.h breeding_rows
        self.S = max(self.breeding, self.parents)                          # ... selected_rows
        # enum sots_sort_mode: "A population outside 1024 < P <= 131072 or with S > P/2 is sorted in full"
        self.selection = 1024 < self.P <= 131072 and 2 * self.S <= self.P
        self.ops = self.graph[0] if self.graph else 0

    def make(self, pkg):
        kw = {}
        if self.graph:
            kw = dict(graph=pkg.capi.make_voice_graph(*self.graph), feedback_genes=self.feedback_genes)
        return pkg.HipES(self.parents, self.offspring, synth_kind=self.kind, audio_log2=self.log2n, param_max=self.pmax,
                         seed=0x5EED0001, workgroup_size=self.block, **kw)


LANDSCAPE = ("set_target_audio", "set_target_spectrum", "set_objective", "set_objective_weights", "set_survivors",
             "set_synth_arithmetic", "set_voice_waveforms", "set_voice_feedback")
READS = ("read_population", "read_population_other", "read_fitness", "read_target", "pack_elites", "best_ever", "history",
         "getters", "read_select_splitters", "read_select_lists", "timing_enable", "timing_reset")
RENDERS = ("render_overlap_add", "render_continuous", "render_graph_genes")
SELECTION = ("set_sort_mode", "set_select_plan", "write_select_splitters", "bucket_fitness", "select")
STAGES = ("recombine", "mutate", "synthesise", "window", "fft", "fitness", "sort", "rotate")
# what B must never see
NOT_FOR_B = set(READS) | set(RENDERS) | set(SELECTION) | {"execute_generations", "execute_until", "refuse", "final_lazy"}
GROUPS = {
    "generation": STAGES,
    "evaluate_sort": STAGES[2:],
    "offspring": STAGES[:6],
    "sort_rotate": STAGES[6:],
}
SPLITTER_SLOTS = ("zero", "ones", "constant", "descending", "one_huge", "nan_region", "garbage")
FLOORS = (1e-3, 1e-6)
REFUSALS = [  # (call, args, code): sots_hip.h's SOTS_ERR_* for each
    ("set_sort_mode", (3,), -1), ("set_select_plan", (3,), -1), ("set_objective", (2, 0.0), -1),
    ("set_objective", (LOG, 2.0), -1), ("set_objective", (LOG, 1e-31), -1), ("set_objective_weights", ("wrong_size",), -1),
    ("write_population", ("wrong_size", 0), -4), ("write_select_splitters", ("wrong_size", 0), -4),
    ("set_survivors", ("parents_plus_one",), -1), ("pack_elites", ("S_plus_one",), -5), ("execute_generations", (1,), -5),
]


class Model:
    """The facts the header documents, as the generator keeps them"""

    def __init__(self, shape):
        self.sh = shape
        self.target = None          # (form, index)
        self.populated = False
        self.mode, self.plan = SORT_LAZY, PLAN_AUTO
        self.pending = False        # a selection's rest is outstanding and the unsorted half intact
        self.overwritten = False    # ... was outstanding under TOP_ONLY when a write ended the state
        self.objective, self.weights, self.survivors, self.arith = (MAGNITUDE, 0.0), None, 0, 0
        self.waveforms, self.feedback = None, None
        self.track = None           # (best_ever, history_every, capacity)
        self.taken = 0              # history records since the last clear, a lower bound
        self.wrapped = False
        self.timing = False
        self.stats = {k: 0 for k in SITUATIONS}
        self.between = None         # kinds of the calls since the last fused generation call; None before the first
        self.splitters_written = False
        self.cycle = 0              # situation l: 0 nothing, 1 on + generations, 2 off + generations

    @property
    def unspecified(self):
        return self.pending and self.mode == SORT_TOP

    def rows(self):
        return self.sh.S if self.unspecified else self.sh.P

    def ready(self):
        return self.target is not None and self.populated

    # -- transitions --
    def clear_record(self):
        self.taken, self.wrapped = 0, False

    def note(self, kind):
        if self.between is not None:
            self.between.append(kind)

    def wrote_rows(self):
        """a call that writes rows ends the pending state (LAZY: the rest is produced first)"""
        if self.pending and self.mode == SORT_TOP:
            self.overwritten = True
        self.pending = False

    def looked(self):
        """a call that looks at rows S..P-1: LAZY produces them, TOP_ONLY keeps the state"""
        if self.pending:
            self.stats["a"] += 1
            if self.mode != SORT_TOP:
                self.pending = False

    def records(self, n):
        if self.track and self.track[1]:
            self.taken += n // self.track[1]
            if self.taken > self.track[2] and not self.wrapped:
                self.wrapped = True
                self.stats["m"] += 1

    def generations(self, n, fused):
        if fused:
            b = self.between
            if b is not None:
                reads = any(k == "read" for k in b)
                self.stats["f"] += "landscape" in b and not reads
                self.stats["g"] += "plan" in b and self.sh.selection
                self.stats["j"] += "refuse" in b
                self.stats["k"] += "render" in b
            self.stats["h"] += self.splitters_written and self.sh.selection
            self.between, self.splitters_written = [], False
            self.pending = self.sh.selection and self.mode != SORT_FULL
            self.overwritten = False
        else:
            self.wrote_rows()
            self.note("generation")
        self.records(n)
        if self.track and self.cycle == 0:
            self.cycle = 1
        elif not self.track and self.cycle == 1:
            self.cycle = 2
        elif self.track and self.cycle == 2:
            self.cycle = 0
            self.stats["l"] += 1


def generate(shape_name, seed, n_ops=OPS):
    """(operations, statistics): n_ops calls, the last one a checkpoint (followed by final_lazy where it applies)"""
    sh = Shape(shape_name)
    rng = np.random.default_rng([seed, len(shape_name)])
    m = Model(sh)
    ops = []
    boundaries = []  # indices after which a replay may stop (a group of stage calls is not cut)

    def ri(lo, hi):  # inclusive
        return int(rng.integers(lo, hi + 1))

    def pick(seq):
        return seq[ri(0, len(seq) - 1)]

    def emit(*op):
        ops.append(tuple(op))

    def setter(current, value):
        m.stats["n"] += current == value
        m.note("landscape")

    # ---- the draws; each returns False where it is not legal now ----
    def d_target():
        form, i = pick(("set_target_audio", "set_target_spectrum")), ri(0, 2)
        setter(m.target, (form, i))
        m.target = (form, i)
        m.clear_record()
        emit(form, i)

    def d_objective():
        if m.objective[0] == LOG and rng.random() < 0.6:  # another floor under LOG (situation o), or the same one again
            kind, floor = LOG, pick(FLOORS)
        else:
            kind = pick((MAGNITUDE, LOG, LOG))
            floor = pick(FLOORS) if kind == LOG else 0.0
        m.stats["o"] += m.objective[0] == LOG and kind == LOG and floor != m.objective[1]
        setter(m.objective, (kind, floor))
        m.objective = (kind, floor)
        m.clear_record()
        emit("set_objective", kind, floor)

    def d_weights():
        w = pick((None, "band", "fixed"))
        setter(m.weights, w)
        m.weights = w
        m.clear_record()
        emit("set_objective_weights", w)

    def d_survivors():
        n = pick((0, 1, sh.parents))
        setter(m.survivors, n)
        m.survivors = n
        emit("set_survivors", n)

    def d_arith():
        if sh.kind == SYNTH_GRAPH:
            return False
        a = ri(0, 1)
        setter(m.arith, a)
        m.arith = a
        emit("set_synth_arithmetic", a)

    def d_voice():
        if sh.kind != SYNTH_GRAPH:
            return False
        if rng.random() < 0.5:
            w = pick((None, (0, 7, 0), (6, 1, 3), (2, 0, 5)))
            setter(m.waveforms, w)
            m.waveforms = w
            emit("set_voice_waveforms", w)
        else:
            f = pick((None, (0.5, 0.0, 0.0), (0.25, 1.5, 0.0)))  # operator 2's index is a gene: its setting stays 0
            setter(m.feedback, f)
            m.feedback = f
            emit("set_voice_feedback", f)
        m.clear_record()

    def room():
        return n_ops - 1 - len(ops)

    def d_init():
        if m.target is None and rng.random() < 0.5:
            return False
        was_pending = m.pending
        m.stats["b"] += m.pending
        m.wrote_rows()
        m.populated = True
        m.clear_record()
        m.note("population")
        emit("init_population", pick((0, 1, 5, 0xFFFFFFFF)))
        if was_pending and room() >= 1 and rng.random() < 0.6:  # the fresh rows, looked at before a generation replaces them
            pick((d_checkpoint, d_read))()

    def d_write():
        what = pick(("whole", "values", "fitness"))
        if what != "whole" and (m.unspecified or not m.populated):
            return False
        m.stats["c"] += m.pending
        m.wrote_rows()
        m.populated = True
        m.note("population")
        emit("write_population", what, ri(0, 999))

    def d_generation_counter():
        m.note("population")
        emit("set_generation", pick(EDGE_GENERATIONS + (0, 3, 0xFFFFFFFE, 0x7FFFFFFF)))

    def d_inject():
        if not m.populated:
            return False
        m.note("population")
        emit("inject_immigrants", ri(1, 4), ri(0, 999))

    def d_fused():
        if not m.ready():
            return False
        n = ri(1, 5)
        m.generations(n, True)
        emit("execute_generations", n)

    def d_staged():
        if not m.ready():
            return False
        m.generations(1, False)
        emit("execute_generation")

    def d_until():
        if not m.ready() or not m.track:
            return False
        check = ri(1, 3)
        max_g = ri(2, 6)
        rule = pick(((1e30, 0), (0.0, 0), (None, 1), (None, 2), (1e-3, 3)))
        m.generations(min(check, max_g), True)  # at least one block
        emit("execute_until", max_g, rule[0], rule[1], check)

    def d_sandwich():
        """execute_generations, one call that is no read, execute_generations"""
        if not m.ready():
            return False
        d_fused()
        between = [d_target, d_objective, d_weights, d_survivors, d_refuse, d_render, d_plan, d_splitters, d_objective]
        while pick(between)() is False:
            pass
        d_fused()

    def d_track_cycle():
        """tracking on, off and on again, generations between (situation l)"""
        if not m.ready() or room() < 6:
            return False
        for new in (pick(((True, 1, 3), (True, 0, 0))), None, pick(((True, 1, 2), (True, 2, 4)))):
            m.track = new
            m.clear_record()
            m.note("track")
            emit("track", *(new or (False, 0, 0)))
            d_fused()

    def d_top_only():
        """a selection under TOP_ONLY whose rest then meets a refused write before the mode is left (situation p), is
        overwritten before it is left (situation e), or is produced by a mode that goes away and comes back; a checkpoint
        looks at what is left"""
        if not m.ready() or not sh.selection or room() < 11:
            return False
        if m.mode != SORT_TOP:
            m.mode = SORT_TOP
            m.note("mode")
            emit("set_sort_mode", SORT_TOP)
        d_fused()
        r = rng.random()
        if r < 0.3:  # a refused write must leave the rest producible: refuse, leave the mode, look (situation p)
            m.stats["p"] += 1
            m.note("refuse")
            emit("refuse", "write_population", ("wrong_size", 0), -4)
            leave = pick((SORT_LAZY, SORT_FULL))
            m.stats["d"] += m.pending
            m.pending = m.overwritten = False
            m.mode = leave
            m.note("mode")
            emit("set_sort_mode", leave)
        elif r < 0.7:
            pick((d_init, d_write_whole, d_offspring))()
            leave = pick((SORT_LAZY, SORT_FULL))
            m.stats["e"] += m.overwritten
            m.stats["d"] += m.pending
            m.overwritten = m.pending = False
            m.mode = leave
            m.note("mode")
            emit("set_sort_mode", leave)
        else:
            away = pick((SORT_LAZY, SORT_FULL))
            m.stats["d"] += m.pending
            m.pending = m.overwritten = False
            m.mode = away
            emit("set_sort_mode", away)
            m.mode = SORT_TOP
            m.note("mode")
            emit("set_sort_mode", SORT_TOP)
        d_checkpoint()

    def d_write_whole():
        m.stats["c"] += m.pending
        m.wrote_rows()
        m.populated = True
        m.note("population")
        emit("write_population", "whole", ri(0, 999))

    def d_offspring():
        m.wrote_rows()
        m.note("generation")
        for s in GROUPS["offspring"]:
            emit(s)

    def d_mode():
        new = pick((SORT_LAZY, SORT_FULL, SORT_TOP, SORT_TOP))
        m.stats["n"] += new == m.mode
        if m.mode == SORT_TOP and new != SORT_TOP:
            m.stats["d"] += m.pending
            m.stats["e"] += m.overwritten
            m.overwritten = False
        if m.pending and new != SORT_TOP:
            m.pending = False  # "leaving SOTS_SORT_TOP_ONLY completes it"; LAZY -> FULL completes it too
        m.mode = new
        m.note("mode")
        emit("set_sort_mode", new)

    def d_plan():
        new = ri(0, 2)
        m.stats["n"] += new == m.plan
        m.plan = new
        m.note("plan")
        emit("set_select_plan", new)

    def d_splitters():
        m.splitters_written = True
        m.note("splitters")
        emit("write_select_splitters", pick(SPLITTER_SLOTS), ri(0, 999))

    def d_unit():
        """bucket_fitness [one call that drops the lists] select rotate; B: sort rotate"""
        if not m.ready() or m.unspecified:
            return False
        m.looked()
        m.note("read")
        emit("bucket_fitness")
        r = rng.random()
        if r < 0.25:
            emit("read_select_lists")
        elif r < 0.8:
            m.stats["i"] += sh.selection
            pick((d_plan, d_splitters, d_target, d_objective, d_weights, d_mode))()
        m.wrote_rows()
        emit("select")
        emit("rotate")
        m.pending = sh.selection and m.mode != SORT_FULL
        m.overwritten = False
        m.note("generation")

    def d_group():
        if not m.ready():
            return False
        name = pick(tuple(GROUPS))
        if m.unspecified and GROUPS[name][0] != "recombine":
            return False
        m.wrote_rows()
        m.note("generation")
        for s in GROUPS[name]:
            emit(s)

    def d_read():
        names = ["read_population", "read_population_other", "read_fitness", "read_target", "pack_elites", "getters",
                 "read_select_splitters", "timing_enable", "timing_reset"]
        if m.track:
            names.append("best_ever")
        if m.track and m.track[1]:
            names.append("history")
        name = pick(names)
        m.note("read")
        if name in ("read_population", "read_fitness"):
            m.looked()
            emit(name)
        elif name == "pack_elites":
            k = pick((1, 16, sh.S, sh.S + 1, sh.P))
            if k > sh.S:
                if m.unspecified:
                    k = sh.S
                else:
                    m.looked()
            emit(name, k)
        elif name == "timing_enable":
            m.timing = not m.timing
            emit(name, m.timing)
        else:
            if m.pending:
                m.stats["a"] += 1  # a read that must leave the pending state alone
            emit(name)

    def d_render():
        m.note("render")
        hop = pick((sh.N // 2, sh.N // 4 + 1, sh.N))
        if sh.kind == SYNTH_GRAPH and rng.random() < 0.6:
            emit("render_graph_genes", 3, hop, ri(0, 99))
        elif sh.kind != SYNTH_GRAPH and m.arith == 0 and rng.random() < 0.5:  # (SOTS_ERR_STATE under SOTS_ARITH_DEVICE_KERNELS)
            emit("render_continuous", 3, hop, ri(0, 99))
        else:
            emit("render_overlap_add", 3, max(hop, (sh.N + 63) // 64), ri(0, 99))

    def d_track():
        new = pick((None, (True, 0, 0), (True, 1, 3), (True, 2, 2), None, (True, 1, 4)))
        if m.track and new is not None and rng.random() < 0.5:
            new = None
        m.track = new
        m.clear_record()
        m.note("track")
        emit("track", *(new or (False, 0, 0)))

    def d_refuse():
        call, args, code = pick(REFUSALS)
        if m.unspecified:  # the refusals that meet a rest outstanding under TOP_ONLY
            r = rng.random()
            if r < 0.35:
                call, args, code = "pack_elites", ("S_plus_one",), -5
            elif r < 0.8:
                call, args, code = "write_population", ("wrong_size", 0), -4
                m.stats["p"] += 1
        if call == "pack_elites" and not m.unspecified:
            return False
        if call == "execute_generations" and m.target is not None:
            return False
        m.note("refuse")
        emit("refuse", call, args, code)

    def d_checkpoint():
        m.note("read")
        emit("checkpoint", m.rows(), bool(m.track), bool(m.track and m.track[1]))
        m.looked()

    draws = [(10, d_fused), (3, d_staged), (4, d_until), (9, d_sandwich), (7, d_mode), (4, d_plan), (2, d_splitters), (8, d_unit),
             (3, d_target), (7, d_objective), (2, d_weights), (2, d_survivors), (2, d_arith), (6, d_voice),
             (4, d_init), (4, d_write), (1, d_generation_counter), (2, d_inject), (3, d_group), (12, d_read), (2, d_render),
             (5, d_track), (5, d_refuse), (5, d_checkpoint),
             (3, d_track_cycle), (7, d_top_only)]  # checkpoints: 5 in 100 draws, under 1 in 8
    weights = np.array([w for w, _ in draws], float)
    start = [(6, d_target), (6, d_init), (1, d_refuse), (1, d_objective), (1, d_track), (1, d_mode)]
    sweights = np.array([w for w, _ in start], float)
    several = (d_sandwich, d_unit, d_group)  # up to 8 calls: not drawn where they would not fit (the others look at room())
    while len(ops) < n_ops - 1:
        table, w = (draws, weights) if m.ready() else (start, sweights)
        if m.pending and rng.random() < 0.45:  # a tail is outstanding: look at it, replace it or change the mode under it
            fn = pick((d_read, d_read, d_init, d_write, d_mode, d_mode, d_checkpoint, d_refuse))
        else:
            fn = table[int(rng.choice(len(table), p=w / w.sum()))][1]
        if fn in several and n_ops - 1 - len(ops) < 8:
            continue
        fn()
        boundaries.append(len(ops))
    assert len(ops) == n_ops - 1
    ops.extend(last_checkpoint(sh, ops))
    return ops, dict(m.stats), boundaries


def last_checkpoint(sh, ops):
    """the checkpoint that ends a list and, where a rest is still outstanding under TOP_ONLY, the switch that produces it"""
    m = replay_model(sh, ops)
    out = [("checkpoint", m.rows(), bool(m.track), bool(m.track and m.track[1]))]
    if m.unspecified:
        out.append(("final_lazy",))
    return out


def replay_model(sh, ops):
    """the facts after `ops`, derived again from the list alone (the generator's own model has seen calls that were cut)"""
    f = FakeContext(sh, role="A")
    for op in ops:
        apply(f, op, sh)
    m = Model(sh)
    m.mode, m.pending = f.mode, f.pending
    m.track = (True, f.tracking[1], f.tracking[2]) if f.tracking[0] else None
    return m


def normalise(ops):
    """B's list: the same logical history by the plainest path"""
    out = []
    for op in ops:
        name = op[0]
        if name == "execute_generations":
            out.extend([("execute_generation",)] * op[1])
        elif name == "execute_until":
            out.append(("b_until",) + op[1:])
        elif name == "select":
            out.append(("sort",))
        elif name in ("checkpoint", "final_lazy"):
            out.append(("checkpoint",) + op[1:] if name == "checkpoint" else ("checkpoint_all",))
        elif name not in NOT_FOR_B:
            out.append(op)
    return out


def cut(shape_name, ops, boundaries, k):
    """the first k operations, extended to the end of a group of stage calls, with a last checkpoint"""
    end = min([b for b in boundaries if b >= k] or [len(ops)])
    head = [op for op in ops[:end] if op[0] != "final_lazy"]
    if head and head[-1][0] == "checkpoint":
        head.pop()
    return head + last_checkpoint(Shape(shape_name), head)


# ---- text ---------------------------------------------------------------------------------------------------------------------
def op_text(op, who="es"):
    name, a = op[0], op[1:]
    if name in ("set_target_audio", "set_target_spectrum"):
        fn = "target_audio" if name == "set_target_audio" else "target_spectrum"
        return f"{who}.{name}(SM.{fn}(sh, {a[0]}))"
    if name == "set_objective_weights":
        return f"{who}.{name}(SM.weights(sh, {a[0]!r}))"
    if name == "write_population":
        return f"{who}.write_population(*SM.population(sh, {a[0]!r}, {a[1]}))"
    if name == "inject_immigrants":
        return f"{who}.inject_immigrants(SM.immigrants(sh, {a[0]}, {a[1]}))"
    if name == "write_select_splitters":
        return f"{who}.write_select_splitters(SM.splitters(sh, {a[0]!r}, {a[1]}, {who}.select_splitter_count()))"
    if name == "set_generation":
        return f"{who}.generation = {a[0]:#x}"
    if name == "execute_until":
        return f"{who}.execute_until({a[0]}, target={a[1]!r}, stall={a[2]}, check_every={a[3]})"
    if name == "b_until":
        return f"SM.until_by_stages({who}, {a[0]}, {a[1]!r}, {a[2]}, {a[3]})"
    if name in RENDERS:
        return f"{who}.{name}(SM.track_rows(sh, {a[0]}, {a[2]}), {a[1]})"
    if name == "track":
        return f"{who}.track({a[0]}, {a[1]}, {a[2]})"
    if name == "refuse":
        return f"SM.refused({who}, sh, {a[0]!r}, {a[1]!r}, {a[2]})"
    if name == "getters":
        return f"SM.getters({who}, sh)"
    if name == "history":
        return f"{who}.history(with_taken=True)"
    if name == "read_population_other":
        return f"{who}.read_population(other=True)"
    if name == "checkpoint":
        return f"# checkpoint: rows 0..{a[0] - 1}, best_ever {a[1]}, history {a[2]}"
    if name == "checkpoint_all":
        return "# checkpoint: every row"
    if name == "final_lazy":
        return f"{who}.set_sort_mode(0)  # and compare every row"
    return f"{who}.{name}({', '.join(repr(x) for x in a)})"


def listing(ops, who="es"):
    return "\n".join(op_text(op, who) for op in ops)


# ---- running a list on anything with HipES's method names ---------------------------------------------------------------------
class Refused(Exception):
    pass


def refused(ctx, sh, call, args, code):
    """the call must fail with `code`; what it leaves behind is for the next checkpoint to find"""
    args = list(args)
    if call == "set_objective_weights":
        args = [np.ones(sh.N // 2 + 1, np.float32)]
    elif call == "write_population":
        args = [np.zeros((sh.P - 1, sh.D), np.float32), None, None]
    elif call == "write_select_splitters":
        args = [np.zeros(ctx.select_splitter_count() + 1, np.uint64)]
    elif call == "set_survivors":
        args = [sh.parents + 1]
    elif call == "pack_elites":
        args = [sh.S + 1]
    try:
        getattr(ctx, call)(*args)
    except Exception as e:  # SotsError of the library, Refused of the fake context
        got = getattr(e, "code", None)
        if got != code:
            raise AssertionError(f"{call}{tuple(args)!r} failed with {got}, expected {code}: {e}")
        return
    raise AssertionError(f"{call}{tuple(args)!r} was not refused (expected {code})")


def getters(ctx, sh):
    """every getter, as arrays of bits"""
    w = ctx.get_objective_weights()
    o = ctx.objective
    out = {"generation": np.array([ctx.generation], np.uint32), "info.generation": np.array([ctx.info().generation], np.uint32),
           "survivors": np.array([ctx.survivors], np.uint32), "objective": np.array([o[0]], np.uint32),
           "floor": np.array([o[1]], np.float32), "weights": np.zeros(0, np.float32) if w is None else np.asarray(w, np.float32)}
    if sh.kind == SYNTH_GRAPH:
        out["waveforms"] = np.array(ctx.voice_waveforms(), np.uint32)
        out["feedback"] = np.array(ctx.voice_feedback(), np.float32)
        out["feedback_genes"] = np.array([ctx.voice_feedback_genes()], np.uint32)
    return out


def until_by_stages(ctx, max_g, target, stall, check_every, holds=None):
    """sots_execute_until as its header states it, on single staged generations: blocks of check_every, after each the
    best-ever record and sots_stop_rule_holds.  The best-ever read is the one read B makes outside a checkpoint; under
    SORT_FULL there is nothing a read could complete."""
    done = 0
    while done < max_g:
        block = min(check_every, max_g - done)
        for _ in range(block):
            ctx.execute_generation()
        done += block
        _, _, f, g = ctx.best_ever()
        if (holds or stop_rule_holds)(ctx, target, stall, check_every, f, g, ctx.generation):
            break
    return done


def stop_rule_holds(ctx, target, stall, check_every, fitness, best_generation, generation):
    """sots_stop_rule_holds of the library the context came from"""
    if isinstance(ctx, FakeContext):
        return True
    import ctypes
    import sys
    capi = sys.modules[type(ctx).__module__]
    rule = capi.make_stop_rule(target, stall, check_every)
    rc = ctx.L.sots_stop_rule_holds(ctypes.byref(rule), ctypes.c_float(float(fitness)), int(best_generation), int(generation))
    assert rc in (0, 1), rc
    return rc == 1


def apply(ctx, op, sh):
    """one operation on ctx; returns what the call returned"""
    name, a = op[0], op[1:]
    if name == "set_target_audio":
        return ctx.set_target_audio(target_audio(sh, a[0]))
    if name == "set_target_spectrum":
        return ctx.set_target_spectrum(target_spectrum(sh, a[0]))
    if name == "set_objective_weights":
        return ctx.set_objective_weights(weights(sh, a[0]))
    if name == "write_population":
        return ctx.write_population(*population(sh, a[0], a[1]))
    if name == "inject_immigrants":
        return ctx.inject_immigrants(immigrants(sh, a[0], a[1]))
    if name == "write_select_splitters":
        return ctx.write_select_splitters(splitters(sh, a[0], a[1], ctx.select_splitter_count()))
    if name == "set_generation":
        ctx.generation = a[0]
        return None
    if name == "execute_until":
        return ctx.execute_until(a[0], target=a[1], stall=a[2], check_every=a[3])
    if name == "b_until":
        return until_by_stages(ctx, *a)
    if name in RENDERS:
        return getattr(ctx, name)(track_rows(sh, a[0], a[2]), a[1])
    if name == "refuse":
        return refused(ctx, sh, a[0], a[1], a[2])
    if name == "getters":
        return getters(ctx, sh)
    if name == "history":
        return ctx.history(with_taken=True)
    if name == "read_population_other":
        return ctx.read_population(other=True)
    if name == "final_lazy":
        return ctx.set_sort_mode(SORT_LAZY)
    if name in ("checkpoint", "checkpoint_all"):
        if isinstance(ctx, FakeContext):
            ctx.checkpointing = True
        try:
            return snapshot(ctx, sh, *(a if name == "checkpoint" else (sh.P, False, False)))
        finally:
            if isinstance(ctx, FakeContext):
                ctx.checkpointing = False
    return getattr(ctx, name)(*a)


def snapshot(ctx, sh, rows, best_ever, history):
    """what a checkpoint compares, as named arrays"""
    v, s, f = ctx.read_population()
    out = {"values": v[:rows], "steps": s[:rows], "fitness": f[:rows], "target": ctx.read_target()}
    out.update(getters(ctx, sh))
    if best_ever:
        bv, bs, bf, bg = ctx.best_ever()
        out.update({"best_ever.values": bv, "best_ever.steps": bs, "best_ever.fitness": np.array([bf], np.float32),
                    "best_ever.generation": np.array([bg], np.uint32)})
    if history:
        h, taken = ctx.history(with_taken=True)
        out.update({"history": h, "history.taken": np.array([taken], np.uint64)})
    return out


def first_difference(a, b):
    """None, or (array name, row) of the first array that differs bit for bit (NaN equal to NaN by its bits)"""
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape:
            return k, -1
        if x.size == 0:
            continue
        rows = max(1, x.shape[0])
        xb, yb = x.view(np.uint8).reshape(rows, -1), y.view(np.uint8).reshape(rows, -1)
        bad = np.flatnonzero((xb != yb).any(axis=1))
        if bad.size:
            return k, int(bad[0])
    return None


# ---- the named arrays ---------------------------------------------------------------------------------------------------------
def target_audio(sh, i):
    n = np.arange(sh.N, dtype=np.float64)
    f0, f1, a1 = [(440.0, 1320.0, 0.3), (1450.0, 200.0, 0.6), (95.0, 5100.0, 0.15)][i]
    x = 0.7 * np.sin(2 * np.pi * f0 * n / 44100.0 + a1 * np.sin(2 * np.pi * f1 * n / 44100.0)) + a1 * np.sin(2 * np.pi * f1 * n / 44100.0)
    return x.astype(np.float32)


def target_spectrum(sh, i):
    n = sh.N
    w = 1.0 - np.cos(2 * np.pi * np.arange(n) / n)
    return (np.abs(np.fft.rfft(target_audio(sh, i).astype(np.float64) * w))[:n // 2] / n / 1.5).astype(np.float32)


def weights(sh, name):
    if name is None:
        return None
    half = sh.N // 2
    if name == "band":
        w = np.zeros(half, np.float32)
        w[half // 8:half // 2] = 1.0
        return w
    from _weights_model import fixed_weights
    return fixed_weights(sh.N)


def population(sh, what, seed):
    rng = np.random.default_rng([7, seed])
    v = rng.random((sh.P, sh.D), dtype=np.float32)
    s = rng.random((sh.P, sh.D), dtype=np.float32) * np.float32(0.1)
    f = rng.random(sh.P, dtype=np.float32)
    f[rng.integers(0, sh.P, 8)] = f[0]          # ties: the row index decides
    f[rng.integers(0, sh.P, 2)] = np.float32("nan")  # NaN rows sort last
    return {"whole": (v, s, f), "values": (v, None, None), "fitness": (None, None, f)}[what]


def immigrants(sh, n, seed):
    rng = np.random.default_rng([11, seed])
    return rng.random((n, 2 * sh.D + 1), dtype=np.float32)


def splitters(sh, name, seed, count):
    """the slots of test_gpu_select_splitters.degenerate, made without a look at the fitness"""
    rng = np.random.default_rng([13, seed])
    one = np.uint64(0x3F800000 | 0x80000000) << np.uint64(32)  # the ordered bits of 1.0f
    if name == "zero":
        return np.zeros(count, np.uint64)
    if name == "ones":
        return np.full(count, 0xFFFFFFFFFFFFFFFF, np.uint64)
    if name == "constant":
        return np.full(count, one, np.uint64)
    if name == "descending":
        return (np.linspace(int(one), int(one) // 2, count).astype(np.uint64))
    if name == "one_huge":
        return (np.uint64(0x80000000) << np.uint64(32)) + np.arange(count, dtype=np.uint64) * np.uint64(1 << 40)
    if name == "nan_region":
        return (np.uint64(0xFFFFFFFD) << np.uint64(32)) | rng.integers(0, sh.P, count).astype(np.uint64)
    return rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2)


def track_rows(sh, rows, seed):
    return np.random.default_rng([17, seed]).random((rows, sh.D), dtype=np.float32)


# ---- a context that computes nothing and objects to what the rules forbid -----------------------------------------------------
class Illegal(AssertionError):
    pass


class FakeContext:
    """HipES's method names on the state the C code keeps (sort_mode, tail_pending, tail_first, target_set ...), written from
    sots_capi.hip and not from the generator's Model.  It records every call, refuses what the library refuses, and raises
    Illegal on a call whose result the header leaves unspecified - and, as role "B", on every call B must not see."""

    def __init__(self, sh, role="A"):
        self.sh, self.role, self.calls = sh, role, []
        self.P, self.D, self.N = sh.P, sh.D, sh.N
        self.mode, self.plan = (SORT_FULL, PLAN_TILES) if role == "B" else (SORT_LAZY, PLAN_AUTO)
        self.target_set = self.populated = False
        self.pending, self.tail_first = False, 0
        self.tail_defined = True     # rows S..P-1 of the current half hold what the full sort would have put there
        self._generation = 0
        self.tracking = (False, 0, 0)
        self.obj, self.w, self._survivors, self.arith = (MAGNITUDE, 0.0), None, 0, 0
        self.waves, self.fb = [0] * sh.ops, [0.0] * sh.ops
        self.audio = self.spectrum = self.fitness_of = None  # which rows' audio / spectrum / fitness the buffers hold
        self.rows_id = 0                                      # changes whenever rows of the current half change
        self.lists_ready = False
        self.selected = False        # sots_stage_select has run, sots_stage_rotate not yet
        self.checkpointing = False   # B reads at checkpoints only

    def _call(self, name, *a):
        if self.role == "B" and name in NOT_FOR_B and not self.checkpointing:
            raise Illegal(f"B must not see {name}")
        if self.selected and name not in ("rotate",):
            raise Illegal(f"{name} between sots_stage_select and sots_stage_rotate")
        self.calls.append((name,) + a)

    def _refuse(self, code, text):
        e = Refused(text)
        e.code = code
        raise e

    def _need_target(self):
        if not self.target_set:
            self._refuse(-5, "no target")

    def _complete(self):  # complete_tail
        if self.pending and self.mode != SORT_TOP:
            self.pending, self.tail_defined = False, True

    def _settle(self):  # settle_tail
        self._complete()
        self.pending = False
        self.lists_ready = False

    def _reads_all_rows(self, name):
        if not self.tail_defined:
            raise Illegal(f"{name} reads rows S..P-1, which SORT_TOP_ONLY left unspecified")

    def _new_rows(self):
        self.rows_id += 1

    # -- setters --
    def set_target_audio(self, a):
        self._call("set_target_audio")
        assert a.shape == (self.N,)
        self.target_set, self.lists_ready = True, False

    def set_target_spectrum(self, m):
        self._call("set_target_spectrum")
        assert m.shape == (self.N // 2,)
        self.target_set, self.lists_ready = True, False

    def set_objective(self, kind, floor=0.0):
        if kind > LOG or (kind == LOG and not (1e-30 <= floor <= 1.0)):
            self._refuse(-1, "objective")
        self._call("set_objective", kind, floor)
        self.obj, self.lists_ready = (kind, floor if kind == LOG else 0.0), False

    def set_objective_weights(self, w):
        if w is not None and w.shape != (self.N // 2,):
            self._refuse(-1, "weights")
        self._call("set_objective_weights")
        self.w, self.lists_ready = w, False

    def set_survivors(self, n):
        if n > self.sh.parents:
            self._refuse(-1, "survivors")
        self._call("set_survivors", n)
        self._survivors = n

    def set_synth_arithmetic(self, a):
        if self.sh.kind == SYNTH_GRAPH:
            raise Illegal("device-kernel arithmetic is not for the graph voice")
        self._call("set_synth_arithmetic", a)
        self.arith = a

    def set_voice_waveforms(self, w):
        if self.sh.kind != SYNTH_GRAPH:
            raise Illegal("waveforms on a fixed voice")
        self._call("set_voice_waveforms", w)
        self.waves, self.lists_ready = list(w or [0] * self.sh.ops), False

    def set_voice_feedback(self, f):
        if self.sh.kind != SYNTH_GRAPH or (f and f[2] != 0.0):
            raise Illegal("feedback setting on a fixed voice or on the gene operator")
        self._call("set_voice_feedback", f)
        self.fb, self.lists_ready = list(f or [0.0] * self.sh.ops), False

    def set_sort_mode(self, mode):
        if mode > SORT_TOP:
            self._refuse(-1, "sort mode")
        self._call("set_sort_mode", mode)
        self.mode, self.lists_ready = mode, False
        self._complete()

    def set_select_plan(self, plan):
        if plan > PLAN_SPLITTERS:
            self._refuse(-1, "plan")
        self._call("set_select_plan", plan)
        self.plan, self.lists_ready = plan, False

    def select_splitter_count(self):
        return 256

    def write_select_splitters(self, keys):
        if keys.shape != (256,):
            self._refuse(-4, "splitters")
        self._call("write_select_splitters")
        self.lists_ready = False

    # -- population --
    def init_population(self, chunk=0):
        self._call("init_population", chunk)
        self.populated, self.pending, self.tail_defined, self._generation = True, False, True, 0
        self.lists_ready = False
        self._new_rows()
        self.fitness_of = self.rows_id

    def write_population(self, values=None, steps=None, fitness=None):
        for x, shape in ((values, (self.P, self.D)), (steps, (self.P, self.D)), (fitness, (self.P,))):
            if x is not None and x.shape != shape:
                self._refuse(-4, "population bytes")
        self._call("write_population")
        whole = values is not None and steps is not None and fitness is not None
        if not whole and not self.populated:
            raise Illegal("a partial write_population into a population nobody made")
        self._settle()
        if not whole:
            self._reads_all_rows("a partial write_population")
        self.tail_defined = self.populated = True
        self._new_rows()
        self.fitness_of = self.rows_id  # (values without fitness: the old fitness, the same in A and B, stays theirs)

    def inject_immigrants(self, rows):
        if rows.shape[0] > self.sh.breeding:
            self._refuse(-1, "immigrants")
        self._call("inject_immigrants", rows.shape[0])
        self._new_rows()
        self.fitness_of = self.rows_id

    @property
    def generation(self):
        return self._generation

    @generation.setter
    def generation(self, g):
        self._call("set_generation", g)
        self._generation = g & 0xFFFFFFFF

    # -- generations --
    def _generation_done(self):
        self._new_rows()
        self.fitness_of = self.rows_id
        self.audio = self.spectrum = None
        self._generation = (self._generation + 1) & 0xFFFFFFFF

    def execute_generations(self, n):
        self._need_target()
        self._call("execute_generations", n)
        self._fused(n)

    def _fused(self, n):
        if not self.populated:
            raise Illegal("generations of a population nobody made")
        self.lists_ready = False
        for _ in range(n):
            self._generation_done()
        select = self.sh.selection and self.mode != SORT_FULL
        self.pending, self.tail_defined, self.tail_first = select, not select, self.sh.S

    def execute_generation(self):
        self._need_target()
        self._call("execute_generation")
        for s in STAGES:
            getattr(self, s)()

    def execute_until(self, max_generations, target=None, stall=0, check_every=32):
        if not self.tracking[0]:
            self._refuse(-5, "tracking is off")
        self._need_target()
        self._call("execute_until", max_generations, target, stall, check_every)
        run = min(check_every, max_generations)  # the fake's best-ever record holds at the first look
        self._fused(run)
        return run

    # -- stages --
    def recombine(self):
        self._call("recombine")
        if not self.populated:
            raise Illegal("recombine of a population nobody made")
        self._settle()
        self.tail_defined = True  # reads whole parent blocks only, writes every row
        self._new_rows()

    def mutate(self):
        self._call("mutate")
        self._settle()
        self._reads_all_rows("mutate")
        self._new_rows()

    def synthesise(self):
        self._call("synthesise")
        self._settle()
        self._reads_all_rows("synthesise")
        self.audio = ("raw", self.rows_id)

    def window(self):
        self._call("window")
        self._settle()
        if self.audio != ("raw", self.rows_id):
            raise Illegal("window without a synthesis of these rows in front of it (the fused loop leaves other audio than the staged one)")
        self.audio = ("windowed", self.rows_id)

    def fft(self):
        self._call("fft")
        self._settle()
        if self.audio != ("windowed", self.rows_id):
            raise Illegal("fft of audio that is not these rows' windowed synthesis")
        self.spectrum = self.rows_id

    def fitness(self):
        self._call("fitness")
        self._settle()
        self._need_target()
        if self.spectrum != self.rows_id:
            raise Illegal("fitness before a spectrum was made since the audio changed")
        self.fitness_of = self.rows_id

    def sort(self):
        self._call("sort")
        self._settle()
        self._reads_all_rows("sort")
        if self.fitness_of != self.rows_id:
            raise Illegal("sort by a fitness that is not these rows'")
        self.sorted_next = True

    def bucket_fitness(self):
        self._call("bucket_fitness")
        self._complete()
        self._reads_all_rows("bucket_fitness")
        self.lists_ready = True

    def read_select_lists(self):
        self._call("read_select_lists")
        if not self.lists_ready:
            self._refuse(-5, "no keys filed")

    def select(self):
        self._call("select")
        self._settle()
        self._reads_all_rows("select")
        if self.fitness_of != self.rows_id:
            raise Illegal("select by a fitness that is not these rows'")
        self.selected = True
        self.sorted_next = True

    def rotate(self):
        self._call("rotate")
        if not getattr(self, "sorted_next", False):
            raise Illegal("rotate without a sort or a selection in front of it")
        select = self.selected and self.sh.selection and self.mode != SORT_FULL
        self.selected = self.sorted_next = False
        self.lists_ready = False
        self._new_rows()
        self.fitness_of = self.rows_id
        self.pending, self.tail_defined, self.tail_first = select, not select, self.sh.S
        self._generation = (self._generation + 1) & 0xFFFFFFFF

    # -- reads --
    def read_population(self, other=False):
        self._call("read_population_other" if other else "read_population")
        if not other:
            self._complete()
        z = np.zeros((self.P, self.D), np.float32)
        return z, z, np.zeros(self.P, np.float32)

    def read_fitness(self):
        self._call("read_fitness")
        self._complete()
        return np.zeros(self.P, np.float32)

    def read_target(self):
        self._call("read_target")
        return np.zeros(self.N // 2, np.float32)

    def pack_elites(self, k):
        if self.pending and k > self.tail_first and self.mode == SORT_TOP:
            self._refuse(-5, "pack_elites under TOP_ONLY")
        self._call("pack_elites", k)
        if self.pending and k > self.tail_first:
            self._complete()
        if k > self.sh.S:
            self._reads_all_rows("pack_elites")

    def read_select_splitters(self):
        self._call("read_select_splitters")

    def timing_enable(self, on=True):
        self._call("timing_enable", on)

    def timing_reset(self):
        self._call("timing_reset")

    def track(self, best_ever=True, history_every=0, capacity=1024):
        self._call("track", best_ever, history_every, capacity)
        self.tracking = (bool(best_ever or history_every), history_every, capacity)

    def best_ever(self):
        if not self.tracking[0]:
            raise Illegal("best_ever with tracking off")
        if self.role == "A":  # (B reads it inside until_by_stages)
            self._call("best_ever")
        return np.zeros(self.D, np.float32), np.zeros(self.D, np.float32), np.float32(0), 0

    def history(self, with_taken=False):
        if not self.tracking[1]:
            raise Illegal("history with the history off")
        self._call("history")
        return np.zeros(0, np.uint32), 0

    def _render(self, name, values, hop):
        self._call(name)
        assert values.shape[1] == self.D and 1 <= hop <= self.N

    def render_overlap_add(self, values, hop):
        if hop < (self.N + 63) // 64:
            raise Illegal("overlap-add hop below ceil(N / 64)")
        self._render("render_overlap_add", values, hop)

    def render_continuous(self, values, hop):
        if self.sh.kind == SYNTH_GRAPH or self.arith:
            raise Illegal("render_continuous on the graph voice or under device-kernel arithmetic")
        self._render("render_continuous", values, hop)

    def render_graph_genes(self, values, hop):
        if self.sh.kind != SYNTH_GRAPH:
            raise Illegal("render_graph_genes on a fixed voice")
        self._render("render_graph_genes", values, hop)

    # -- getters --
    @property
    def survivors(self):
        return self._survivors

    @property
    def objective(self):
        return self.obj

    def get_objective_weights(self):
        return self.w

    def info(self):
        class I:
            generation = self._generation
        return I

    def voice_waveforms(self):
        return self.waves

    def voice_feedback(self):
        return self.fb

    def voice_feedback_genes(self):
        return self.sh.feedback_genes or 0


# =================================================================================================================================
# The batch (sots_batch_*): a smaller machine.  The subject is one HipBatch; the reference is one HipES per chunk driven
# through the same logical history, as tests/test_gpu_batch.py's sequential() does, and for queue runs the sequential
# tracked context that the header of sots_batch_queue_run spells out.  The two advance in lockstep (run_batch): under
# SOTS_ANALYSIS_DEVICE the reference's targets are the batch's own analyse_audio_hop output, as tests/test_gpu_analysis.py
# has it.  Legality, from include/sots_hip.h:
#   * "Sets the number of ACTIVE chunks": generations and reads need targets, and need every active chunk's population made
#     since the count last grew (a chunk that was inactive kept its rows but missed the batch's generation counter) - the
#     generator asks for init_population whenever the count grows or shrinks and grows again.
#   * sots_batch_queue_run: "Afterwards the batch has NO active targets": set_target_* and init_population come again.
#   * sots_batch_queue_run "needs SOTS_TRACK_BEST_EVER on the batch and fails with SOTS_TRACK_HISTORY on", "needs targets stored".
BATCH_SHAPES = {
    "shipped": dict(kind=SYNTH_3OP, log2n=11, parents=16, offspring=16, block=16, slots=8,
                    pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]),
    "b2op": dict(kind=SYNTH_2OP, log2n=10, parents=256, offspring=768, block=32, slots=4, pmax=[3520.0, 8.0, 3520.0, 1.0]),
}
BATCH_SEEDS = {name: [4200 + 100 * i + j for j in range(8)] for i, name in enumerate(BATCH_SHAPES)}
BATCH_OPS = 40
HOST, DEVICE = 0, 1
BATCH_READS = ("read_best", "read_population", "best_ever", "history", "analyse_audio_hop", "queue_score_audio_hop",
               "queue_kept_population", "getters")
BATCH_REFUSALS = [("set_target_spectra", ("too_many",), -1), ("set_objective", (2, 0.0), -1), ("set_objective_weights", ("wrong_size",), -1),
                  ("set_survivors", ("parents_plus_one",), -1), ("execute_generations", (1,), -5), ("queue_run", (0, 2), -5),
                  ("read_population", ("beyond_active",), -1), ("set_analysis", (2,), -1), ("queue_set_carry", ("parents_plus_one", 1), -1)]


class BatchShape(Shape):
    def __init__(self, name):
        c = BATCH_SHAPES[name]
        self.name, self.kind, self.log2n = name, c["kind"], c["log2n"]
        self.parents, self.offspring, self.block, self.slots = c["parents"], c["offspring"], c["block"], c["slots"]
        self.pmax, self.graph, self.feedback_genes = c["pmax"], None, None
        self.N, self.P, self.D = 1 << self.log2n, self.parents + self.offspring, len(c["pmax"])
        self.breeding = max(1, self.parents // self.block) * self.block
        self.S, self.selection, self.ops = max(self.breeding, self.parents), False, 0

    def make_batch(self, pkg):
        return pkg.HipBatch(self.slots, self.parents, self.offspring, synth_kind=self.kind, audio_log2=self.log2n, param_max=self.pmax,
                            seed=0x5EED0001, workgroup_size=self.block)


def generate_batch(shape_name, seed, n_ops=BATCH_OPS):
    """(operations, statistics) for a HipBatch; the last operation is a checkpoint"""
    sh = BatchShape(shape_name)
    rng = np.random.default_rng([seed, 77])
    ops = []
    st = dict(active=0, made=0, track=None, queue=None, kept=False, analysis=HOST, carry=(0, 0), objective=(MAGNITUDE, 0.0))
    stats = dict(shrink=0, grow=0, queue_runs=0, refills=0, carried=0, kept=0, device_targets=0, refusals=0, until=0, setter_mid_run=0)

    def ri(lo, hi):
        return int(rng.integers(lo, hi + 1))

    def pick(seq):
        return seq[ri(0, len(seq) - 1)]

    def emit(*op):
        ops.append(tuple(op))

    def runnable():
        return st["active"] > 0 and st["made"] >= st["active"]

    def d_target():
        n = ri(1, sh.slots)
        stats["shrink"] += 0 < n < st["active"]
        stats["grow"] += n > st["active"] > 0
        stats["device_targets"] += st["analysis"] == DEVICE
        st["made"] = min(st["made"], n) if n <= st["active"] else 0
        st["active"] = n
        emit(pick(("set_target_audio", "set_target_spectra")), n, ri(0, 2))

    def d_init():
        if st["active"] == 0:
            return False
        st["made"] = st["active"]
        emit("init_population", pick((0, 3, 0xFFFFFFFE)))

    def d_run():
        if not runnable():
            return False
        emit("execute_generations", ri(1, 4))

    def d_until():
        if not runnable() or not st["track"]:
            return False
        stats["until"] += 1
        rule = pick(((1e30, 0), (0.0, 0), (None, 1), (None, 2)))
        emit("execute_until", ri(2, 6), rule[0], rule[1], ri(1, 3))

    def d_setter():
        stats["setter_mid_run"] += runnable()
        which = ri(0, 2)
        if which == 0:
            kind = pick((MAGNITUDE, LOG, LOG))
            st["objective"] = (kind, pick(FLOORS) if kind == LOG else 0.0)
            emit("set_objective", *st["objective"])
        elif which == 1:
            emit("set_objective_weights", pick((None, "band", "fixed")))
        else:
            emit("set_survivors", pick((0, 1, sh.parents)))

    def d_track():
        st["track"] = pick((None, (True, 0, 0), (True, 0, 0), (True, 1, 3), (True, 2, 2)))
        emit("track", *(st["track"] or (False, 0, 0)))

    def d_queue():
        m = pick((1, 3, sh.slots, sh.slots + 1, sh.slots + 3, 2 * sh.slots + 1))
        st["queue"] = m
        st["kept"] = False
        stats["device_targets"] += st["analysis"] == DEVICE
        emit(pick(("queue_targets_audio", "queue_targets_spectra")), m, ri(0, 2))

    def d_carry():
        st["carry"] = pick(((0, 0), (1, 2), (sh.parents, 3), (2, 1), (1, 99)))
        emit("queue_set_carry", *st["carry"])

    def d_queue_run():
        if not st["queue"] or not st["track"] or st["track"][1]:
            return False
        keep = pick((None, ri(0, st["queue"] - 1), ri(0, st["queue"] - 1)))
        rule = pick(((None, 0), (1e30, 0), (None, 1), (0.0, 0)))
        stats["queue_runs"] += 1
        stats["refills"] += st["queue"] > sh.slots
        stats["carried"] += st["carry"][0] > 0 and st["carry"][1] > 1 and st["queue"] > 1
        stats["kept"] += keep is not None
        st["kept"] = keep is not None
        st["active"] = st["made"] = 0
        emit("queue_run", pick((0, 5)), ri(2, 5), rule[0], rule[1], ri(1, 2), keep)

    def d_analysis():
        st["analysis"] = ri(0, 1)
        emit("set_analysis", st["analysis"])

    def d_read():
        names = ["analyse_audio_hop", "getters"]
        if runnable():
            names += ["read_best", "read_population"]
            if st["track"]:
                names.append("best_ever")
            if st["track"] and st["track"][1]:
                names.append("history")
        if st["queue"]:
            names.append("queue_score_audio_hop")
        if st["kept"]:
            names.append("queue_kept_population")
        name = pick(names)
        if name in ("read_population", "history"):
            emit(name, ri(0, st["active"] - 1))
        elif name == "analyse_audio_hop":
            emit(name, ri(1, 5), pick((sh.N, sh.N // 2, 1, 37)), ri(0, 2))
        elif name == "queue_score_audio_hop":
            emit(name, st["queue"], pick((sh.N, sh.N // 4)), ri(0, 2))
        else:
            emit(name)

    def d_refuse():
        call, args, code = pick(BATCH_REFUSALS)
        if call == "execute_generations" and st["active"]:
            return False
        if call == "queue_run" and st["queue"] and st["track"] and not st["track"][1]:
            return False
        if call == "read_population" and not st["active"]:
            return False
        stats["refusals"] += 1
        emit("refuse", call, args, code)

    def d_checkpoint():
        emit("checkpoint", st["active"] if runnable() else 0, bool(st["track"]), bool(st["track"] and st["track"][1]))

    draws = [(8, d_run), (4, d_until), (5, d_target), (5, d_init), (4, d_setter), (4, d_track), (4, d_queue), (5, d_carry),
             (9, d_queue_run), (2, d_analysis), (8, d_read), (3, d_refuse), (3, d_checkpoint)]
    w = np.array([x for x, _ in draws], float)
    while len(ops) < n_ops - 1:
        if st["active"] and not runnable() and rng.random() < 0.6:
            d_init()
            continue
        draws[int(rng.choice(len(draws), p=w / w.sum()))][1]()
    d_checkpoint()
    return ops, stats


def batch_signal(sh, i, samples):
    """a long signal whose N-sample chunks all differ: two partials that glide"""
    n = np.arange(samples, dtype=np.float64)
    f0, f1 = [(300.0, 2.0e-3), (900.0, -1.0e-3), (150.0, 5.0e-3)][i]
    phase = 2 * np.pi * (f0 * n + 0.5 * f1 * f0 * n * n / 1000.0) / 44100.0
    return (0.6 * np.sin(phase) + 0.3 * np.sin(2.7 * phase + 1.0)).astype(np.float32)


def batch_spectra(sh, i, chunks):
    a = batch_signal(sh, i, chunks * sh.N).astype(np.float64).reshape(chunks, sh.N)
    w = 1.0 - np.cos(2 * np.pi * np.arange(sh.N) / sh.N)
    return (np.abs(np.fft.rfft(a * w, axis=1))[:, :sh.N // 2] / sh.N / 1.5).astype(np.float32)


CHUNK_FIELDS = ("generations_run", "best_ever_generation", "best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values")


def run_batch(batch, refs, sh, ops, new_result):
    """the list on the batch and, in lockstep, on one context per chunk (refs[c]; refs[0] also serves the queue runs: after a
    run the batch needs its targets and populations again, so nothing of chunk 0 is lost).  None, or (operation index, text)
    of the first difference.  new_result(n): a zeroed array of n chunk results."""
    analysis = HOST
    queue = None      # per chunk: ("audio", samples) or ("spectrum", magnitudes), as the reference takes it
    carry = (0, 0)
    kept = None

    def same(got, want, what, i):
        d = first_difference(got, want)
        return None if d is None else (i, f"{what}: {d[0]!r} differs, first at row {d[1]}")

    def targets_of(form, n, sig):
        """what the batch is given, and what each reference is given"""
        if form == "spectra":
            m = batch_spectra(sh, sig, n)
            return m, [("spectrum", m[c]) for c in range(n)]
        a = batch_signal(sh, sig, n * sh.N)
        if analysis == DEVICE:  # the device's magnitudes are not the host's bits: the references get the device's
            m = batch.analyse_audio_hop(a, sh.N, n)
            return a, [("spectrum", m[c]) for c in range(n)]
        return a, [("audio", a[c * sh.N:(c + 1) * sh.N]) for c in range(n)]

    def give(ctx, t):
        (ctx.set_target_audio if t[0] == "audio" else ctx.set_target_spectrum)(t[1])

    for i, op in enumerate(ops):
        name, a = op[0], op[1:]
        if name in ("set_target_audio", "set_target_spectra"):
            x, per = targets_of("spectra" if name == "set_target_spectra" else "audio", a[0], a[1])
            getattr(batch, name)(x.reshape(a[0], -1))
            for c in range(a[0]):
                give(refs[c], per[c])
        elif name == "init_population":
            batch.init_population(a[0])
            for c in range(batch.active):
                refs[c].init_population((a[0] + c) & 0xFFFFFFFF)
        elif name == "execute_generations":
            batch.execute_generations(a[0])
            for c in range(batch.active):
                refs[c].execute_generations(a[0])
        elif name == "execute_until":
            max_g, target, stall, check = a
            got = batch.execute_until(max_g, target=target, stall=stall, check_every=check)
            done = 0
            while done < max_g:  # "the first block boundary at which the rule holds for EVERY active chunk"
                block = min(check, max_g - done)
                for c in range(batch.active):
                    refs[c].execute_generations(block)
                done += block
                if all(stop_rule_holds(refs[c], target, stall, check, *refs[c].best_ever()[2:], refs[c].generation) for c in range(batch.active)):
                    break
            if got != done:
                return i, f"execute_until ran {got} generations, the sequential contexts {done}"
        elif name in ("set_objective", "set_survivors", "track"):
            getattr(batch, name)(*a)
            for r in refs:
                getattr(r, name)(*a)
        elif name == "set_objective_weights":
            batch.set_objective_weights(weights(sh, a[0]))
            for r in refs:
                r.set_objective_weights(weights(sh, a[0]))
        elif name in ("queue_targets_audio", "queue_targets_spectra"):
            x, queue = targets_of("spectra" if name == "queue_targets_spectra" else "audio", a[0], a[1])
            getattr(batch, name)(x.reshape(a[0], -1))
            kept = None
        elif name == "queue_set_carry":
            batch.queue_set_carry(*a)
            carry = a
        elif name == "set_analysis":
            batch.set_analysis(a[0])
            analysis = a[0]
        elif name == "queue_run":
            first, max_g, target, stall, check, keep = a
            got, stats = batch.queue_run(first, max_g, target=target, stall=stall, check_every=check, keep=keep)
            es, want = refs[0], new_result(len(queue))
            no_rule = (target is None or target < 0) and not stall
            for k, t in enumerate(queue):  # the header's sequence, carried rows included
                successor = carry[0] > 0 and k % carry[1] != 0
                if successor:
                    pv, ps, _ = es.read_population()
                    bv, bs, _, _ = es.best_ever()
                give(es, t)
                es.init_population((first + k) & 0xFFFFFFFF)
                if successor:
                    v, s, _ = es.read_population()
                    v[:carry[0]], s[:carry[0]] = pv[:carry[0]], ps[:carry[0]]
                    v[0], s[0] = bv, bs
                    es.write_population(v, s, None)
                if no_rule:
                    es.execute_generations(max_g)
                    run = max_g
                else:
                    run = es.execute_until(max_g, target=target, stall=stall, check_every=check)
                bv, bs, bf, bg = es.best_ever()
                pop = es.read_population()
                r = want[k]
                r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = run, bg, bf, pop[2][0]
                r["best_ever_values"][:sh.D], r["best_ever_steps"][:sh.D], r["last_values"][:sh.D] = bv, bs, pop[0][0]
                if keep == k:
                    kept = pop
            bad = same({f: got[f] for f in CHUNK_FIELDS}, {f: want[f] for f in CHUNK_FIELDS}, "queue results", i)
            if bad:
                return bad
            if stats["chunk_generations"] != int(want["generations_run"].sum()):
                return i, "queue statistics: chunk_generations is not the sum of generations_run"
            if keep is not None:
                bad = same(dict(zip("vsf", batch.queue_kept_population())), dict(zip("vsf", kept)), "kept population", i)
                if bad:
                    return bad
        elif name == "queue_kept_population":
            bad = same(dict(zip("vsf", batch.queue_kept_population())), dict(zip("vsf", kept)), "kept population, read again", i)
            if bad:
                return bad
        elif name == "read_best":
            batch.read_best()
        elif name == "read_population":
            batch.read_population(a[0])
        elif name == "best_ever":
            batch.best_ever()
        elif name == "history":
            batch.history(a[0], with_taken=True)
        elif name == "getters":
            batch.get_analysis(), batch.queue_carry()
        elif name == "analyse_audio_hop":
            sig = batch_signal(sh, a[2], (a[0] - 1) * a[1] + sh.N)
            m1, m2 = batch.analyse_audio_hop(sig, a[1], a[0]), batch.analyse_audio_hop(sig, a[1], a[0])
            bad = same({"m": m1}, {"m": m2}, "analyse_audio_hop twice", i)
            if bad:
                return bad
        elif name == "queue_score_audio_hop":
            batch.queue_score_audio_hop(batch_signal(sh, a[2], (a[0] - 1) * a[1] + sh.N), a[1], a[0])
        elif name == "refuse":
            call, args, code = a
            args = list(args)
            if call == "set_target_spectra":
                args = [np.zeros((sh.slots + 1, sh.N // 2), np.float32)]
            elif call == "read_population":
                args = [batch.active]
            elif call == "queue_set_carry":
                args = [sh.parents + 1, 1]
            active = batch.active
            refused(batch, sh, call, args, code)
            batch.active = active  # (the wrapper's own count: a refused target call changes nothing in the library)
        elif name == "checkpoint":
            n, best, hist = a
            if n:
                v, f = batch.read_best()
                be = batch.best_ever() if best else None
                for c in range(n):
                    got = dict(zip(("values", "steps", "fitness"), batch.read_population(c)))
                    want = dict(zip(("values", "steps", "fitness"), refs[c].read_population()))
                    got["best.values"], got["best.fitness"] = v[c], f[c:c + 1]
                    want["best.values"], want["best.fitness"] = want["values"][0], want["fitness"][:1]
                    if best:
                        rv, rs, rf, rg = refs[c].best_ever()
                        got.update({"best_ever.values": be[0][c], "best_ever.steps": be[1][c], "best_ever.fitness": be[2][c:c + 1],
                                    "best_ever.generation": be[3][c:c + 1]})
                        want.update({"best_ever.values": rv, "best_ever.steps": rs, "best_ever.fitness": np.array([rf], np.float32),
                                     "best_ever.generation": np.array([rg], np.uint32)})
                    if hist:
                        h, taken = batch.history(c, with_taken=True)
                        rh, rtaken = refs[c].history(with_taken=True)
                        got.update({"history": h, "taken": np.array([taken], np.uint64)})
                        want.update({"history": rh, "taken": np.array([rtaken], np.uint64)})
                    bad = same(got, want, f"checkpoint, chunk {c}", i)
                    if bad:
                        return bad
        else:
            raise AssertionError(f"unknown operation {op!r}")
    return None

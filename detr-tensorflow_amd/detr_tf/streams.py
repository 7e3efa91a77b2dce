"""The engine's two extra launch streams, one owner each: SideStream (work that does not feed the critical chain) and DropMasks
(the keep bits of the attention-probability dropout).  Both are built once in DetrEngine.__init__."""
import torch

from . import _hip as hip


class SideStream:
    """Work that does not feed the critical chain is issued on a second HIP stream behind an event of the main stream that
    follows its producer (a graph edge when the pass is captured) and is joined where its result is read:
      backward: every weight gradient (it feeds nothing but the bucket exchange / the optimiser) and the data gradient of a
                stage's projection shortcut; forward: the projection shortcut and the decoder's shared K / V projection.
    They share the chip with the chain: the decoder's 800-row kernels fill a fifth of the CUs, the backbone's HBM-bound 1x1
    GEMMs leave the MFMA pipes idle.  The tensors a side launch reads are never rewritten within the same pass (suffix(): one
    scratch tensor per site instead of one per shape; the backbone loop guards its recycled tensors with mark() / wait()), so
    the only joins are in front of a reduction flush, a bucket hand-over, the consumer of a shortcut / of K, V, and the end of
    the pass.  Off (begin(False): DETR_HIP_WGRAD_STREAM=0, and any backward with immediate split-K reductions): run() calls
    inline, everything else does nothing."""

    def __init__(self, device):
        self.on = False
        self.main = None                                # the stream the pass is issued on (set by begin)
        self.side = torch.cuda.Stream(device=device)
        self._marks = {}

    def begin(self, on):
        self.on = bool(on)
        self._marks.clear()
        hip.AFTER_FLUSH = self.sync_both if self.on else None
        if self.on:
            self.main = torch.cuda.current_stream()

    def end(self):
        """End of the pass: join, then off."""
        try:
            self.join()
        finally:
            self.begin(False)

    def run(self, fn):
        if not self.on:
            fn()
            return
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            fn()

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)

    def sync_both(self):
        """After a reduction flush the slab pool is recycled: whichever stream ran the flush, the other one must not write a
        recycled slab before the flush has read it."""
        if self.on:
            self.main.wait_stream(self.side)
            self.side.wait_stream(self.main)

    def suffix(self, site):
        """Suffix that makes a scratch tensor private to one site while the second stream is in use."""
        return f":{site}" if self.on else ""

    def event(self):
        """An event behind everything issued on the side stream so far (None when off)."""
        if not self.on:
            return None
        ev = torch.cuda.Event()
        ev.record(self.side)
        return ev

    def mark(self, key):
        """Remember the side stream's position under `key` (the backbone backward: one per block)."""
        if self.on:
            self._marks[key] = self.event()

    def wait(self, key):
        """The main stream waits for the position marked as `key`, once; an unknown key is nothing to wait for."""
        ev = self._marks.pop(key, None)
        if ev is not None:
            self.main.wait_event(ev)


class DropMasks:
    """Keep bits of the attention-probability dropout (hip.attention_dropmask; bf16 compute mode only): one buffer per site and
    step parity, filled by one launch on a stream of their own -- by gen() at the head of their step, or one step ahead by
    pregen() / at_matcher() (eager launches only) -- and joined in front of the first attention that reads them.
    Every eager launch leaves an event on the mask stream; settle() makes the main stream wait for it before the launch's inputs
    (the device seed block) or outputs (a mask buffer about to be replaced) are touched there."""

    def __init__(self, engine, heads):
        self.eng, self.heads = engine, heads
        self.stream = torch.cuda.Stream(device=engine.device)
        self.set = 0              # parity of the buffer set the current step reads
        self.tags = {}            # parity -> (step seed, B, L, Q, p) of the bits it holds
        self.pending = False      # a launch of this step has not been joined yet
        self.deferred = None      # (B, L) of a generation ahead that waits for the matcher hook
        self.busy = None          # event behind the last eager launch on the mask stream

    def active(self):
        return self.eng.attn16 and self.eng._drop[0] > 0.0

    def sites(self, L):
        e = self.eng
        sites = [(16 * i, L, L) for i in range(e.num_enc)]
        for i in range(e.num_dec):
            ds = 16 * (32 + i)
            sites += [(ds, e.Q, e.Q), (ds + 2, e.Q, L)]
        return sites

    def mask(self, site, B, T, S, which=None):
        """The keep-bit buffer of `site` in set `which` (default: the current step's)."""
        name = f"dropmask:{self.set if which is None else which}:{site}"
        words = hip.attention_dropmask_words(B, self.heads, T, S)
        old = self.eng._bufs.get(name)
        if old is not None and old.numel() != words:
            self.settle()         # the launch that fills the old buffer may still be queued (never inside a capture: the eager step before a recording has sized them)
        return self.eng.buf(name, (words,), torch.int32)

    def settle(self):
        """Order the current stream behind the last launch on the mask stream (an already satisfied wait in the normal case)."""
        if self.busy is not None:
            torch.cuda.current_stream().wait_event(self.busy)
            self.busy = None

    def _launch(self, B, L, which, seed_slot):
        e = self.eng
        main = torch.cuda.current_stream()
        bufs = [(self.mask(site, B, T, S, which), T, S, site) for site, T, S in self.sites(L)]      # (allocated on the main stream)
        self.stream.wait_stream(main)
        with torch.cuda.stream(self.stream):
            hip.attention_dropmask_many(bufs, B, self.heads, dropout_p=e._drop[0], dropout_step=e._seed_dev[seed_slot:])
            if not e._graph_replay:       # (a captured launch is ordered by the graph's own edges)
                self.busy = torch.cuda.Event()
                self.busy.record()

    def gen(self, B, L):
        """The keep-bit buffers of this step's attention sites: already there when the previous step generated them one step ahead,
        otherwise generated now behind the seed write (they depend on nothing else)."""
        e = self.eng
        if not self.active():
            return
        self.set = e._step_no & 1
        key = (e._step_seed, B, L, e.Q, e._drop[0])
        if not (self.tags.get(self.set) == key and not e._graph_replay):
            self._launch(B, L, self.set, 0)
            self.tags[self.set] = None if e._graph_replay else key
        self.pending = True

    def pregen(self, B, L, ahead):
        """Called when the decoder forward begins (800-row kernels, then the matcher: most CUs idle for ~1.5 ms): the NEXT step's keep
        bits, from its seed in slot 1 of the device seed block, into the other buffer set.  Eager launches only (a recorded graph keeps
        the generation at the head of its own step).  ahead = engine.DROPMASK_AHEAD: 2 (the default) launches them from the matcher
        hook (at_matcher), next to the assignment kernel alone (one wave per problem, ~50 CUs for ~0.7 ms); 1 launches them here, next
        to the decoder's chain of short launches (which the co-running generator slowed: +0.07 ms per step,
        profiles/r06_ab_results.txt #3); 0 turns the generation ahead off."""
        if not self.active() or self.eng._graph_replay or not ahead:
            return
        if ahead == 2:
            self.deferred = (B, L)
        else:
            self._ahead(B, L)

    def at_matcher(self):
        args, self.deferred = self.deferred, None
        if args is not None:
            self._ahead(*args)

    def _ahead(self, B, L):
        e = self.eng
        nxt = (e._step_no + 1) & 1
        self._launch(B, L, nxt, 1)
        self.tags[nxt] = (e.seed_of_step(e._step_no + 1), B, L, e.Q, e._drop[0])

    def join(self):
        if self.pending:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.pending = False

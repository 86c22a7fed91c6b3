"""Records the ORDER of what Trainer.step does, at seams that outlive a restructuring of step() itself
(tests/test_gpu_step_order.py, tests/dist_child.py).  install() wraps them and returns a Recorder; every event is a tuple:

    ("run", name)                  Trainer._run, name as passed (before the /warmup and /inj suffixes)
    ("reduce", "g" | "d", "captured" | "inline", part, carry)
                                   the outermost FlatGradSync.all_reduce_captured / all_reduce, while parallel.is_dist()
    ("wait", "g" | "d")            FlatGradSync.wait with a handle that is not None
    ("sync_buffers",)              parallel.sync_buffers while is_dist()
    ("fetch",)                     Trainer.fetch_reals
    ("ema",)                       gans.trainer.ema_inplace
    ("adam", "G" | "D")            Trainer._opt_step
    ("tail", ada_due)              parallel.tail_exchange

Under graph replay the events inside a body do not occur: that is part of the trace."""
import functools


class Recorder:
    def __init__(self):
        self.events = []
        self._undo = []
        self._depth = 0   # > 0 inside a recorded reduction: all_reduce_captured calls all_reduce

    def take(self):
        """The events since the last take(), as JSON would hold them (lists, not tuples)."""
        ev, self.events = self.events, []
        return [list(e) for e in ev]

    def _wrap(self, owner, name, before):
        orig = getattr(owner, name)

        @functools.wraps(orig)
        def wrapped(*a, **kw):
            before(*a, **kw)
            return orig(*a, **kw)
        setattr(owner, name, wrapped)
        self._undo.append((owner, name, orig))

    def _wrap_reduce(self, cls, name, kind, sig):
        from gans import parallel
        orig = getattr(cls, name)
        rec = self

        @functools.wraps(orig)
        def wrapped(sync, *a, **kw):
            if rec._depth == 0 and parallel.is_dist():
                args = dict(zip(sig, a), **kw)
                rec.events.append(("reduce", _which(sync), kind, args.get("part"), bool(args.get("carry", False))))
            rec._depth += 1
            try:
                return orig(sync, *a, **kw)
            finally:
                rec._depth -= 1
        setattr(cls, name, wrapped)
        self._undo.append((cls, name, orig))

    def uninstall(self):
        for owner, name, orig in reversed(self._undo):
            setattr(owner, name, orig)
        self._undo = []


def _which(sync):
    return "g" if type(sync.module).__name__ == "Generator" else "d"


def install():
    import gans.trainer as T
    from gans import parallel
    rec = Recorder()
    ev = lambda e: rec.events.append(e)   # noqa: E731  (take() re-binds rec.events: append through the attribute)
    rec._wrap(T.Trainer, "_run", lambda tr, name, fn, *args: ev(("run", name)))
    rec._wrap_reduce(parallel.FlatGradSync, "all_reduce_captured", "captured", ("part", "carry"))
    rec._wrap_reduce(parallel.FlatGradSync, "all_reduce", "inline", ("async_op", "part", "carry"))
    rec._wrap(parallel.FlatGradSync, "wait", lambda sync, handle: handle is not None and ev(("wait", _which(sync))))
    rec._wrap(parallel, "sync_buffers", lambda *a, **kw: parallel.is_dist() and ev(("sync_buffers",)))
    rec._wrap(T.Trainer, "fetch_reals", lambda *a, **kw: ev(("fetch",)))
    rec._wrap(T, "ema_inplace", lambda *a, **kw: ev(("ema",)))
    rec._wrap(T.Trainer, "_opt_step", lambda tr, opt: ev(("adam", "G" if opt is tr.optim_G else "D")))
    rec._wrap(parallel, "tail_exchange",
              lambda named, ada_stats=None, module=None: ev(("tail", ada_stats is not None)))
    return rec

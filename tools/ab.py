"""The measuring protocol behind the tools/*_bench.py scripts, in one place: device-event timing, the median/min/max
summary, alternated rounds over two or more arms with the toggled module flag restored whatever happens, the three
rules that turn two summaries into a verdict, the model train step with a flag on and off, and the JSON-lines output
with the common command-line block.  A tool keeps what is particular to it -- the operation, the shapes and why, which
rule decides its exit status -- and takes the rest from here.  (hosts/harness.py keeps its own loop: that one is the
reference's model_benchmark protocol, not this one.)

Importing this module also puts the package directory on sys.path, so `import ab` comes before `from tome import ...`."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "video-how-do-your-tokens-merge_amd"))

DEV = "cuda:0"
PEAK_TBS = 8.0  # HBM3E peak of one MI355X, TB/s: what `share_of_8TBps` divides by


def time_us(fn, iters, warmup=0, sync=True, cuda=torch.cuda):
    """Microseconds per call of `fn` over `iters` calls between two device events, after `warmup` untimed calls (and,
    if there were any and `sync`, a device synchronise, so the timed calls start on an idle queue).  `cuda` is the
    namespace the events and the synchronise come from; the CPU tests pass a fake one."""
    for _ in range(warmup):
        fn()
    if warmup and sync:
        cuda.synchronize()
    start, stop = cuda.Event(enable_timing=True), cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def switch_arms(module, attr):
    """The two arms of a module flag, native (True) first."""
    return {True: (module, attr, True), False: (module, attr, False)}


def _with_arm(arm, fn, do):
    """do(run) with `run` the arm's callable: the arm itself, or `fn` under the arm's (module, attr, value) setting."""
    if callable(arm):
        return do(arm)
    module, attr, value = arm
    before = getattr(module, attr)
    setattr(module, attr, value)
    try:
        return do(fn)
    finally:
        setattr(module, attr, before)


def alternate(arms, rounds, iters, fn=None, warm="call", time=time_us):
    """{name: [us per call, one per round]} over `arms` = {name: callable | (module, attr, value) applied around `fn`},
    the native arm first.  Every arm is warmed once, in order, then `rounds` x (every arm in order) are timed.
    `warm`: "call" (one bare call), a count n (`time(run, n)`), or a callable warm(name, run) for a tool that measures
    something of its own while it warms up (peak memory, launches per step)."""
    def warm_up(name, run):
        if callable(warm):
            warm(name, run)
        elif warm == "call":
            run()
        else:
            time(run, warm)

    for name, arm in arms.items():
        _with_arm(arm, fn, lambda run: warm_up(name, run))
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, arm in arms.items():
            times[name].append(_with_arm(arm, fn, lambda run: time(run, iters)))
    return times


def held_between(paths, g):
    """(held, warm): a warm-up for `alternate` over arms named as `paths` = {name: forward callable} that also records
    in held[name] the bytes a path keeps allocated between its forward and its backward, the output aside."""
    held = {}

    def warm(name, run):
        run()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = paths[name]()
        torch.cuda.synchronize()
        held[name] = torch.cuda.memory_allocated() - base - out.numel() * out.element_size()
        out.backward(g)

    return held, warm


def larger_spread(a, b):
    return max(a["max_us"] - a["min_us"], b["max_us"] - b["min_us"])


def tie_within_spread(native, other):
    """"tie" when the native median is not above the other's by more than the larger of the two min-max spreads."""
    return "tie" if native["median_us"] <= other["median_us"] + larger_spread(native, other) else "native slower"


def median_below_median(native, other):
    return native["median_us"] < other["median_us"]


def median_below_fastest(native, other):
    return native["median_us"] < other["min_us"]


def tie_report(times, what, other="framework"):
    """The fields of a tie-rule comparison of times[True] (native) with times[False] (`other`)."""
    nat, oth = summary(times[True]), summary(times[False])
    return {"native_" + what: nat, other + "_" + what: oth, "larger_spread_us": round(larger_spread(nat, oth), 1),
            "native_over_" + other + "_median": round(nat["median_us"] / oth["median_us"], 3),
            "verdict": tie_within_spread(nat, oth)}


def launch_alone(fn, rounds, iters):
    """One launch on its own, no arms: a call to warm up, then `rounds` timings."""
    fn()
    return [time_us(fn, iters) for _ in range(rounds)]


def bandwidth(launch, nbytes):
    """The summary of `launch` with `nbytes` over its unrounded median."""
    tbps = nbytes / statistics.median(launch) / 1e6
    return dict(summary(launch), bytes=nbytes, TBps=round(tbps, 2), share_of_8TBps=round(tbps / PEAK_TBS, 3))


def model_train_step(make, patch, clip_shape, batch, r, switch, rounds, iters, warm, dtype=None, autocast=None,
                     **patch_kw):
    """{True: [...], False: [...]}: one forward + backward of a patched host in .train(), `switch` = (module, attr) on
    and off in alternated rounds.  The model and the clip are cast to `dtype` if given (the 16-bit hosts); the forward
    runs under torch.autocast(`autocast`) if given (fp32 master weights)."""
    torch.manual_seed(0)
    model = make().to(DEV).to(dtype).train()  # (.to(None) is a no-op)
    patch(model, **patch_kw)
    model.r = r
    clip = torch.rand(batch, *clip_shape, device=DEV).to(dtype)

    def forward():
        if autocast is None:
            return model([clip])
        with torch.autocast("cuda", dtype=autocast):
            return model([clip])

    def step():
        model.zero_grad(set_to_none=True)
        forward().float().square().sum().backward()

    return alternate(switch_arms(*switch), rounds, iters, fn=step, warm=warm)


def parser(iters=10, out=None):
    """The command-line block every A/B tool has; a tool adds its own flags to what this returns."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=out, help="also write the JSON lines to this file")
    return ap


class Lines:
    """The JSON lines of one run: printed as they come, kept, written to `out` at the end."""

    def __init__(self, out):
        self.out, self.lines = out, []

    def emit(self, res):
        self.lines.append(json.dumps(res))
        print(self.lines[-1], flush=True)

    def write(self):
        if self.out:
            os.makedirs(os.path.dirname(os.path.abspath(self.out)), exist_ok=True)
            with open(self.out, "w") as f:
                f.write("\n".join(self.lines) + "\n")

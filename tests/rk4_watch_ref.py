"""The rules of the monitored fixed-step RK4 loop (csrc/marl_rk4_watch_ctl.h) restated in Python: the step epilogue one lane of the
workgroup runs, the frame-list check, and a driver that steps the CPU oracle's RK4 under those rules - the reference the tests of the
kernel, of the header and of the sweep driver share."""
import numpy as np

DONE, TERMINAL, NONFINITE = 0, 1, -2
FRAME, STOP = 1, 2
SLOT = (1, 2, 3, 5, 6, 4, 7)        # record slot of monitor e (rk45_monitor_of_record)


def monitor(rec, e):
    return rec[SLOT[e]] - 1.0 if e in (3, 4) else rec[SLOT[e]]


def record_of_events(g, bad=0.0):
    """the reduction record {count, min y, min CA, min CC, min U, max CA+CC, max Phi, max W} whose monitors are g"""
    rec = np.zeros(8)
    rec[0] = bad
    for e in range(7):
        rec[SLOT[e]] = g[e] + 1.0 if e in (3, 4) else g[e]
    return rec


def check_frames(frame_steps, nsteps):
    """index of the first entry that is not a strictly ascending step count in [0, nsteps]; -1: none"""
    for j, k in enumerate(frame_steps):
        if k < 0 or k > nsteps or (j > 0 and k <= frame_steps[j - 1]):
            return j
    return -1


class Watch:
    """Rk4WatchRec and its two functions"""

    def __init__(self, t0, dt, rec, frame_steps=(), lim=None, max_events=None):
        self.t0, self.dt, self.t = float(t0), float(dt), float(t0)
        self.frame_steps, self.lim, self.max_events = list(frame_steps), lim, max_events
        self.g = [monitor(rec, e) for e in range(7)]
        self.n_events = [0] * 7
        self.t_events = [[] for _ in range(7)]          # the stored ones: at most max_events each (None: the caller passed no buffer)
        self.steps, self.next_frame, self.status = 0, 0, DONE
        self.begin = 0
        if self.frame_steps and self.frame_steps[0] == 0:
            self.next_frame, self.begin = 1, FRAME

    def time(self, s):
        return self.t0 + np.float64(s) * self.dt

    def step(self, rec):
        s = self.steps
        t_old, t_new = self.time(s), self.time(s + 1)
        self.steps, self.t = s + 1, float(t_new)
        if not rec[0] == 0.0:
            self.status = NONFINITE
            return STOP
        out = 0
        for e in range(7):
            go, gn = self.g[e], monitor(rec, e)
            if (go <= 0.0 and gn >= 0.0) or (go >= 0.0 and gn <= 0.0):
                d = go - gn
                tc = t_old + self.dt * (go / d) if d != 0.0 else t_new
                if self.max_events is not None and self.n_events[e] < self.max_events:
                    self.t_events[e].append(float(tc))
                self.n_events[e] += 1
                if self.lim is not None and self.lim[e] > 0 and self.n_events[e] == self.lim[e]:
                    self.status = TERMINAL
                    out |= STOP
            self.g[e] = gn
        if self.next_frame < len(self.frame_steps) and self.frame_steps[self.next_frame] == s + 1:
            self.next_frame += 1
            out |= FRAME
        return out


def oracle_record(P, N, y):
    """the reduction record of a state by the CPU oracle's monitors; slot 0 counts the cells with a non-finite field"""
    from oracle import oracle as orc
    y = np.asarray(y, dtype=float)
    bad = float(np.count_nonzero(~np.all(np.isfinite(y.reshape(5, N)), axis=0)))
    with np.errstate(all="ignore"):
        g = np.asarray(orc.events(P, N, y), dtype=float)
    return record_of_events(g, bad)


def oracle_run(P, N, y0, dt, nsteps, t0=0.0, frame_steps=(), lim=None, max_events=None):
    """The watched run on the CPU oracle: one orc.rk4 step at a time under the rules above.
    Returns (Watch, y_final, {frame index: state})."""
    from oracle import oracle as orc
    y = np.array(y0, dtype=float)
    w = Watch(t0, dt, oracle_record(P, N, y), frame_steps, lim, max_events)
    frames = {0: y.copy()} if w.begin & FRAME else {}
    for _ in range(nsteps):
        with np.errstate(all="ignore"):
            y = orc.rk4(P, N, y, dt, 1)
        dec = w.step(oracle_record(P, N, y))
        if dec & FRAME:
            frames[w.next_frame - 1] = y.copy()
        if dec & STOP:
            break
    return w, y, frames

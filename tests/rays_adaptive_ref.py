"""Shared inputs of the ray-accumulator tests (tests/test_rays_adaptive_host.py
on the host, tests/test_gpu_rays_adaptive.py on the GPU) — TEST
INFRASTRUCTURE.  A batch of 192 ray records per scene, the oracle's per-sample
colours of every record (rays_ref.ray_samples: sample s of a record is one
oracle call on the descriptor with eye = o), and the numpy simulation of the
two stop rules on them (adaptive_sim.simulate), each computed once per process
and shared.

The aimed batch: with lo, hi the box of the object triangles' vertices,
c = (lo+hi)/2 and h = (hi-lo)/2, the targets are
T = (c.x + 0.9 h.x u, c.y + 0.9 h.y v, c.z) for u, v in linspace(-1, 1, 12),
x outer.  Record i starts at rays_ref.OFF_AXIS[0], the scene's eye or
rays_ref.OFF_AXIS[1] (i mod 3), crosses z = 0 at
p = o.xy + (T.xy - o.xy) * (o.z / (o.z - T.z)) and has key 7 i mod 4096.  The
first 48 records of rays_ref.batch(pk, 257) follow, for escapes and light
hits.  The scene's ray box is the box of every origin but OFF_AXIS[1], which
stays outside it."""
import numpy as np

import adaptive_sim
import rays_ref

BOUNCES, SEED = 3, 9
N_AIMED, N_TAIL = 144, 48
# (tol, floor, min_spp, max_spp, step_spp)
RULES = {"r4-32-4": (0.05, 0.01, 4, 32, 4), "r3-17-5": (0.1, 0.01, 3, 17, 5)}
MAX_SPP = 32
# the preconditions a comparison against the simulation rests on
MIN_MARGIN = 1e-4


def aimed_batch(pk, tail_seed=7):
    """(o, p, d, keys) of the 192 records."""
    v = np.asarray(pk.tri_v, dtype=np.float64).reshape(-1, 3)[:3 * pk.n_obj_tri]
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    eye = np.array([float(x) for x in pk.eye])
    origins = (np.array(rays_ref.OFF_AXIS[0]), eye, np.array(rays_ref.OFF_AXIS[1]))
    lin = np.linspace(-1.0, 1.0, 12)
    o = np.zeros((N_AIMED, 3))
    p = np.zeros((N_AIMED, 2))
    i = 0
    for u in lin:
        for w in lin:
            T = np.array([c[0] + 0.9 * h[0] * u, c[1] + 0.9 * h[1] * w, c[2]])
            o[i] = origins[i % 3]
            p[i] = o[i, :2] + (T[:2] - o[i, :2]) * (o[i, 2] / (o[i, 2] - T[2]))
            i += 1
    keys = ((7 * np.arange(N_AIMED)) % 4096).astype(np.uint32)
    bo, bp, _, bk = rays_ref.batch(pk, 257, seed=tail_seed)
    o = np.concatenate([o, bo[:N_TAIL]])
    p = np.concatenate([p, bp[:N_TAIL]])
    keys = np.concatenate([keys, bk[:N_TAIL]])
    o, d = rays_ref.rays_through(o, p)
    return o, p, d, keys


class Batch:
    """A scene's records, their ray box, the oracle's samples (lazily, per
    Russian-roulette depth) and the simulated runs.  By default the 192 records
    of aimed_batch with rays_ref.ray_samples as the source of the samples;
    `records` = (o, d, keys, box) and `source` = f(rr_depth, ns) -> [ns, n, 3]
    give any other records and reference (tests/rays_any_ref.py: rays that
    cross no screen plane, through oracle.radiance)."""

    def __init__(self, scene, records=None, source=None):
        from pathtracerpython_amd.pack import pack_scene
        self.scene = scene
        self.pk = pack_scene(scene)
        if records is None:
            self.o, self.p, self.d, self.keys = aimed_batch(self.pk)
            inb = ~np.all(self.o == np.array(rays_ref.OFF_AXIS[1]), axis=1)
            self.box = np.concatenate([self.o[inb].min(axis=0), self.o[inb].max(axis=0)])
            self.outside = ~inb
        else:
            assert source is not None
            self.o, self.d, self.keys, self.box = records
            self.p = None
            self.outside = ~np.all((self.o >= self.box[:3]) & (self.o <= self.box[3:]), axis=1)
        self.source = source
        self.n = len(self.o)
        self._samples = {}
        self._sim = {}

    def samples(self, rr_depth=None, ns=MAX_SPP):
        """[ns, n, 3]: the reference's colour of samples 0 .. ns-1 of every record."""
        from pathtracerpython_amd._abi import PT_FLAG_RR
        key = (rr_depth, ns)
        if key not in self._samples:
            if self.source is not None:
                self._samples[key] = self.source(rr_depth, ns)
            else:
                self._samples[key] = rays_ref.ray_samples(
                    self.scene, self.o, self.p, self.keys, BOUNCES, SEED, ns,
                    flags=0 if rr_depth is None else PT_FLAG_RR, rr_depth=3 if rr_depth is None else rr_depth)
        return self._samples[key]

    def simulate(self, rule, rr_depth=None):
        """adaptive_sim.simulate of RULES[rule] on the samples, shape (192,)."""
        key = (rule, rr_depth)
        if key not in self._sim:
            tol, floor, lo, hi, step = RULES[rule]
            self._sim[key] = adaptive_sim.simulate(self.samples(rr_depth), tol, floor, lo, hi, step)
        return self._sim[key]

    def check_preconditions(self, rule, rr_depth=None):
        """What makes the comparison meaningful: no stop decision within 1e-4
        of the threshold (sums that agree to 1e-12 then cannot flip one), and
        records of every kind."""
        sim = self.simulate(rule, rr_depth)
        s = self.samples(rr_depth)
        esc, lit, other = rays_ref.coverage(s, self.pk.light_rgb)
        hist = adaptive_sim.histogram(sim["n"])
        hi = RULES[rule][3]
        print(f"{rule} rr={rr_depth}: counts {hist}, {len(sim['passes'])} passes, margin {sim['margin']:.2e}, "
              f"{esc} all-escape, {lit} all-light, {other} other records")
        assert sim["margin"] >= MIN_MARGIN
        assert esc >= 5 and lit >= 3
        assert len(hist) >= 4
        assert hist.get(hi, 0) >= 10
        return sim


def trajectory(samples, rule):
    """The run of RULES[rule] pass by pass on per-sample colours samples[s]
    (n, 3): a list of (n_active, added, n after the pass).  The moments of a
    select are the samples summed up to the counts (adaptive_sim.moments_upto):
    at a margin >= MIN_MARGIN the decisions are the simulation's."""
    tol, floor, lo, hi, step = RULES[rule]
    n = np.zeros(samples.shape[1], dtype=np.int64)
    out = []
    for _ in range(hi + 1):
        S, Q = adaptive_sim.moments_upto(samples, n)
        act = adaptive_sim.active_numpy(n, adaptive_sim.err_numpy(S, Q, n, floor), tol, lo, hi)
        if not act.any():
            return out
        k = np.where(act, adaptive_sim.k_numpy(n, lo, hi, step), 0)
        n = n + k
        out.append((int(act.sum()), int(k.sum()), n.copy()))
    raise AssertionError("the run did not end")


_batches = {}


def batch_of(name, scene):
    """The process-wide Batch of scene `name` ("cornell" or "mesh")."""
    if name not in _batches:
        _batches[name] = Batch(scene)
    return _batches[name]

"""What the admp_md_* entries promise at the C boundary apart from their arithmetic (include/admp_hip.h; the arithmetic has its
own tests, tests/test_gpu_md_*.py): which entry refuses a slab-decomposed handle with which code and text, and that this refusal
wins over any other defect; what a launch without its plan answers; the three *_info layouts word by word; that the launches
follow the handle's stream of the moment; and the profiler labels.  Raw ctypes calls on handles of both precisions, 3 atoms, one
bond, one constraint, groups [0, 0, 1]."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5                    # include/admp_hip.h
N = 3
BOX = np.diag([20.0, 21.0, 22.0]).reshape(-1)
FIRE_PAR = (0.5, 5.0, 0.01, 0.1, 20.0, 1.1, 0.5, 0.25, 0.99)
TOL, SWEEPS = 1e-6, 10
STATE_REFUSED = ['langevin', 'random', 'bonded_box', 'virial', 'scale', 'mts_plan', 'mts_step', 'con_plan', 'con_step', 'con_kick',
                 'con_project', 'mol_plan', 'mol_sums', 'mol_scale']
NEEDS_PLAN = {'mts_step': 'admp_md_mts_plan must precede admp_md_mts_step',
              'con_step': 'admp_md_con_plan must precede admp_md_con_step',
              'con_kick': 'admp_md_con_plan must precede admp_md_con_kick',
              'con_project': 'admp_md_con_plan must precede admp_md_con_project',
              'mol_sums': 'admp_md_mol_plan must precede admp_md_mol_sums',
              'mol_scale': 'admp_md_mol_plan must precede admp_md_mol_scale'}
LABELS = {'md_bonded', 'md_kick_drift', 'md_langevin', 'md_random', 'md_bonded_box', 'md_virial', 'md_scale', 'md_mts',
          'md_con_step', 'md_con_kick', 'md_con_project', 'md_mol_sums', 'md_mol_scale', 'md_fire'}
# the entry behind each label; the two that scale come late, so that the constraint still holds where it is solved
LAUNCHING = ['bonded', 'kick_drift', 'langevin', 'random', 'bonded_box', 'virial', 'mts_step', 'con_step', 'con_kick',
             'con_project', 'mol_sums', 'scale', 'mol_scale', 'fire_step']


class Handle:
    """a handle of its own (admp_create), the device tensors and host arrays of one valid call of every entry"""

    def __init__(self, nbytes):
        import torch
        from admp_amd import _lib
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        assert self.L.admp_create(ctypes.byref(self.h), 0, nbytes) == 0
        dev = torch.device('cuda', 0)
        real = torch.float32 if nbytes == 4 else torch.float64
        t = lambda a, dtype=real: torch.as_tensor(np.asarray(a), dtype=dtype, device=dev).contiguous()      # noqa: E731
        self.t = {
            'pos': t([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [5.0, 6.0, 7.0]]),      # |r1 - r0| = 1: the bond and the constraint at rest
            'vel': t(np.zeros((N, 3))), 'grad': t(np.zeros((N, 3))), 'grad2': t(np.full((N, 3), 0.5)),
            'ref': t([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [5.0, 6.0, 7.0]]),
            'inv_mass': t(np.ones(N)),
            'bidx': t([[0, 1]], torch.int32), 'bpar': t([[100.0, 1.0]]),
            'words2': t([0.25, 0.5], torch.float64), 'words9': t(np.arange(9.0), torch.float64),
            'words21': t(np.arange(21.0), torch.float64), 'ekin': t([7.0], torch.float64),
            'counters': t([0, 0], torch.int32), 'normals': t(np.full((N, 3), 9.0)),
            'fire_state': t(np.tile([FIRE_PAR[0], FIRE_PAR[7], 0, 0, 0, 0, 0, 0], (2, 1)), torch.float64),
        }
        self.box = _lib.darr(BOX)
        self.fire_par = _lib.darr(FIRE_PAR)
        self.h_bidx = np.array([[0, 1]], dtype=np.int32)
        self.h_bpar = np.array([[100.0, 1.0]])
        self.h_len = np.array([1.0])
        self.h_groups = np.array([0, 0, 1], dtype=np.int32)
        torch.cuda.synchronize()

    def close(self):
        assert self.L.admp_destroy(self.h) == 0

    def entries(self):
        """name -> f(n): the call with valid arguments but for its atom count (bond count for bonded_box), which is n"""
        L, h, b = self.L, self.h, self.box
        p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in self.t.items()}
        hb, hp, hl, hg = (a.ctypes.data for a in (self.h_bidx, self.h_bpar, self.h_len, self.h_groups))
        return {
            'bonded': lambda n: L.admp_md_bonded(h, p['pos'], b, 1, p['bidx'], p['bpar'], 0, None, None, p['words2'], p['grad2']),
            'kick_drift': lambda n: L.admp_md_kick_drift(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], 1e-4, 1.0, p['ekin']),
            'langevin': lambda n: L.admp_md_langevin(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], 1e-4, 1.0, 1.0, 0.0, 1, 0,
                                                     p['ekin']),
            'random': lambda n: L.admp_md_random(h, 1, n, 1, 0, 0, p['normals']),
            'bonded_box': lambda n: L.admp_md_bonded_box(h, p['pos'], b, 1 if n == N else n, p['bidx'], p['bpar'], 0, None, None,
                                                         p['words2'], p['words9']),
            'virial': lambda n: L.admp_md_virial(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], 1, 0, p['words21']),
            'scale': lambda n: L.admp_md_scale(h, n, p['pos'], p['vel'], 2.0),
            'mts_plan': lambda n, tile=0: L.admp_md_mts_plan(h, n, 1, hb, hp, 0, None, None, tile),
            'mts_step': lambda n: L.admp_md_mts_step(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], b, 1e-4, 1.0, 2, 1.0, 0.0, 1,
                                                     0, p['words2'], p['grad2']),
            'con_plan': lambda n, tile=0: L.admp_md_con_plan(h, n, 1, hb, hl, tile),
            'con_step': lambda n: L.admp_md_con_step(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], b, 1e-4, 1.0, 1.0, 0.0, 1, 0,
                                                     TOL, SWEEPS, p['counters']),
            'con_kick': lambda n: L.admp_md_con_kick(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], b, 1e-4, 1.0, TOL, SWEEPS,
                                                     p['ekin'], p['counters']),
            'con_project': lambda n: L.admp_md_con_project(h, n, p['pos'], p['ref'], p['inv_mass'], b, TOL, SWEEPS, p['counters']),
            'mol_plan': lambda n, tile=0: L.admp_md_mol_plan(h, n, hg, tile),
            'mol_sums': lambda n: L.admp_md_mol_sums(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], b, 1, 0, p['words21']),
            'mol_scale': lambda n: L.admp_md_mol_scale(h, n, p['pos'], p['vel'], p['inv_mass'], b, 1.0, -0.5),
            'fire_step': lambda n: L.admp_md_fire_step(h, n, p['pos'], p['vel'], p['grad'], p['inv_mass'], self.fire_par, 0.0, 0,
                                                       p['fire_state']),
        }

    def info(self, which):
        out = (ctypes.c_int64 * 8)(*([-1] * 8))
        assert getattr(self.L, 'admp_md_%s_info' % which)(self.h, out) == 0
        return [int(x) for x in out]

    def infos(self):
        return {w: self.info(w) for w in ('mts', 'con', 'mol')}

    def error(self):
        return self.L.admp_last_error(self.h)

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.t.items()}

    def unchanged_since(self, snap):
        import torch
        assert self.L.admp_synchronize(self.h) == 0
        torch.cuda.synchronize()
        return all(torch.equal(v, snap[k]) for k, v in self.t.items())


@pytest.fixture(params=[8, 4], ids=['double', 'single'])
def handle(request):
    hd = Handle(request.param)
    try:
        yield hd
    finally:
        hd.close()


def test_slab_handle_refused_before_any_other_check(handle):
    """every entry but admp_md_bonded and admp_md_kick_drift (which accept such a handle and are not called here), with valid
    arguments and once more with a negative count: the same refusal both times, nothing planned, nothing launched"""
    assert handle.L.admp_slab_configure(handle.h, 0, 2) == 0
    f = handle.entries()
    assert set(f) == set(STATE_REFUSED) | {'fire_step', 'bonded', 'kick_drift'}      # every entry but the three *_info has a row
    snap = handle.snapshot()
    for name in STATE_REFUSED + ['fire_step']:
        for n in (N, -1):
            rc, msg = f[name](n), handle.error()
            print(name, n, rc, msg)
            assert rc == (E_ARG if name == 'fire_step' else E_STATE), (name, n)
            assert b'single-rank' in msg, (name, n)
            if name == 'fire_step':
                assert msg == b'the MD helpers serve single-rank handles only (slab-decomposed handle)'
            else:
                assert msg == b'the MD helpers serve single-rank handles only'
    assert handle.unchanged_since(snap)
    assert handle.infos() == {'mts': [0] * 8, 'con': [0] * 8, 'mol': [0] * 8}


def test_launch_without_its_plan(handle):
    f = handle.entries()
    snap = handle.snapshot()
    assert handle.infos() == {'mts': [0] * 8, 'con': [0] * 8, 'mol': [0] * 8}
    for name, sentence in NEEDS_PLAN.items():
        rc, msg = f[name](N), handle.error()
        print(name, rc, msg)
        assert rc == E_ARG and msg == sentence.encode(), name
    assert handle.unchanged_since(snap)
    assert handle.infos() == {'mts': [0] * 8, 'con': [0] * 8, 'mol': [0] * 8}


def test_info_layouts(handle):
    """mts: [n_tiles, tile_atoms, max_component, n_atoms, n_bonds, n_angles, lds_bytes, launches]
    con: [n_tiles, tile_atoms, max_cluster, n_atoms, n_cons, n_clusters, lds_bytes, launches]
    mol: [n_tiles, tile_atoms, max_group, n_atoms, n_groups, lds_bytes, threads, launches]
    with the default tile of 256 atoms (256 lanes), then re-planned with tiles of 64 (64 lanes): the launch count survives."""
    f = handle.entries()
    for plan in ('mts_plan', 'con_plan', 'mol_plan'):
        assert f[plan](N) == 0, handle.error()
    first = handle.infos()
    print(first)
    mts, con, mol = first['mts'], first['con'], first['mol']
    assert mts[:6] == [1, 256, 2, N, 1, 0] and mts[6] > 0 and mts[7] == 0
    assert con[:5] == [1, 256, 2, N, 1] and con[5] in (1, 2) and con[6] > 0 and con[7] == 0
    assert mol[:5] == [1, 256, 2, N, 2] and mol[5] > 0 and mol[6] == 256 and mol[7] == 0
    for family, launch in (('mts', 'mts_step'), ('con', 'con_project'), ('mol', 'mol_sums')):
        assert f[launch](N) == 0, handle.error()
        want = {k: list(v) for k, v in first.items()}
        want[family][7] = 1
        assert handle.infos() == want, family      # one launch moves word 7 of its family and nothing else
        first = want
    for plan in ('mts_plan', 'con_plan', 'mol_plan'):
        assert f[plan](N, 64) == 0, handle.error()
    again = handle.infos()
    print(again)
    for family in ('mts', 'con', 'mol'):
        assert again[family][1] == 64 and again[family][7] == 1
        assert again[family][0] == 1 and again[family][2:5] == first[family][2:5]
    assert again['mol'][6] == 64
    assert handle.L.admp_synchronize(handle.h) == 0


def test_launches_follow_the_stream_of_the_moment(handle):
    """A caller's stream before the first MD call, then back to the default stream.  Each time the stream is kept busy, a fill
    of the positions with 1 is queued behind that work, and admp_md_scale by 2 is called: in stream order the positions end
    at 2; a launch on any other stream would find the stream idle, run before the fill and leave 1."""
    import torch
    L, h, pos, vel = handle.L, handle.h, handle.t['pos'], handle.t['vel']
    big = torch.zeros(1 << 26, dtype=torch.float32, device=pos.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=pos.device)
    assert L.admp_set_stream(h, ctypes.c_void_p(s.cuda_stream)) == 0
    scale = handle.entries()['scale']
    for stream in (s, torch.cuda.default_stream(pos.device)):
        if stream is not s:
            assert L.admp_use_default_stream(h) == 0
        with torch.cuda.stream(stream):
            for _ in range(20):
                big.add_(1.0)
            pos.fill_(1.0)
            vel.fill_(1.0)
        assert scale(N) == 0, handle.error()
        stream.synchronize()
        assert bool((pos == 2.0).all()) and bool((vel == 0.5).all())
    torch.cuda.synchronize()


def test_profiler_labels(handle):
    f = handle.entries()
    L, h = handle.L, handle.h
    for plan in ('mts_plan', 'con_plan', 'mol_plan'):
        assert f[plan](N) == 0, handle.error()
    assert L.admp_profile_enable(h, 1) == 0
    for name in LAUNCHING:
        assert f[name](N) == 0, (name, handle.error())
    n = L.admp_profile_count(h)
    seen = {}
    for k in range(n):
        label, ms, count = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
        assert L.admp_profile_entry(h, k, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(count)) == 0
        seen[label.value.decode()] = int(count.value)
    print(seen)
    assert set(seen) == LABELS and n == len(LABELS)
    assert all(c == 1 for c in seen.values())
    assert L.admp_profile_enable(h, 0) == 0

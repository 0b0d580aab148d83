"""MD-driver helpers on the GPU (the reference has no integrator; its drivers stop at get_forces).

`HarmonicBonded` evaluates the bonded terms of the drivers' force field (examples/*/mpidwater.xml:16-21: harmonic O-H bonds
and H-O-H angles) with one HIP kernel over explicit lists (include/admp_hip.h admp_md_bonded); `VelocityVerlet` does the two
half steps with one kernel each (admp_md_kick_drift).  Energies accumulate in device words and are read only when the caller
logs, so an MD step adds no host synchronisation of its own to those of the calculators.  Used by examples/md/nve_water.py.

`Langevin` is the thermostat: BAOAB (Leimkuhler and Matthews 2013) with the same two-call shape, its first half one kernel
(admp_md_langevin) that draws its noise in registers from a counter-based generator (csrc/md_math.h: Philox-4x32-10, a
function of (seed, step, stream, atom) alone, so a restart at any step repeats the noise); `maxwell_boltzmann` draws the
initial velocities from the same generator (admp_md_random).  Used by examples/md/nvt_water.py.

`CRescaleBarostat` is the isotropic barostat: stochastic cell rescaling (Bernetti and Bussi 2020).  One application reads the
two 3x3 sums a pressure needs and its normal from one launch (admp_md_virial), takes dE/dbox summed over the caller's
calculators (`HarmonicBonded.get_box_gradient` is the bonded share, admp_md_bonded_box), and rescales positions, velocities
(admp_md_scale) and the caller's box.  Used by examples/md/npt_water.py.

`MTSLangevin` is the multiple-time-step integrator (impulse r-RESPA with two levels): the bonded terms of a `HarmonicBonded`
advance by n inner BAOAB steps inside one kernel, whole molecules resident in LDS (admp_md_mts_plan / admp_md_mts_step), and
the calculators are called once per outer step.  Used by examples/md/mts_water.py.

`Constraints` holds pairwise distance constraints (rigid water, constrained X-H bonds) and projects positions and velocities
onto them; `ConstrainedLangevin` is constrained BAOAB on them -- SHAKE on the displacement of the first half step, RATTLE on
the velocities of the second, one kernel each with whole clusters resident in LDS (admp_md_con_plan / admp_md_con_step /
admp_md_con_kick / admp_md_con_project).  Used by examples/md/rigid_water.py.

`MolecularCRescaleBarostat` is the barostat for constrained (or any molecular) systems: groups of atoms are scaled as rigid
bodies about their centres of mass and the pressure is the molecular one, so the constraints survive an application without a
re-projection (admp_md_mol_plan / admp_md_mol_sums / admp_md_mol_scale); `groups_of` makes the group labels from the lists of
a `HarmonicBonded` and / or a `Constraints`.  Used by examples/md/npt_water.py --molecular / --rigid.

`FireMinimizer` is the energy minimiser that prepares a start: FIRE (Bitzek et al. 2006) with the half step back of FIRE 2.0
(Guenole et al. 2020) and a hard cap on every atom's move.  One iteration is one C call (admp_md_fire_step) of two kernels: six
sums and maxima in double without atomics, then the decision -- downhill or uphill, the new time step, converged, failed -- taken
on the device from a double-buffered state (csrc/md_fire_math.h), so an iteration reads nothing back and is bit-repeatable; with
a `Constraints` it minimises on them.  Used by examples/md/minimize_water.py and by every driver with --minimizer fire.

`VRescale` is the global thermostat: stochastic velocity rescaling (Bussi, Donadio and Parrinello 2007), the one the two
barostats were designed to run with.  One application is one C call (admp_md_vrescale) of two kernels: the closing half kick of
the step and the kinetic energy in double without atomics, then the draw of the new kinetic energy and the factor on the device
from (seed, step) (csrc/md_vrescale_math.h) and one pass that scales the velocities -- nothing read back, bit-repeatable.  One
factor for all atoms keeps constrained velocities on their constraints, and the state carries the heat the thermostat has put
in, so E_pot + K - heat is conserved.  Used by every driver in examples/md with --thermostat vrescale.

`DipoleRecorder` records the dipole observable along a run: the molecular dipoles' statistics and the cell dipole, split into
charge, permanent-dipole and induced parts, one row of 16 doubles per `record` in a device array (admp_pme_dipoles: two kernels
without atomics, the arithmetic in csrc/dipole_math.h), read when the run ends; `group_csr` turns group labels into the CSR pair
the kernel walks, `dielectric_constant` the rows into the static dielectric constant.  `ADMPPmeForce.get_dipoles` is the same
call with one host read.  Used by every driver in examples/md with --dipoles N.

`RdfRecorder` accumulates radial distribution functions along a run: the typed pair-distance counts of a frame are added to a
device histogram of 64-bit counters by one C call (admp_md_rdf: pairs of 256-atom tiles up to 4096 atoms, a cell sweep above;
integer atomics only, so the counts are bit-identical from run to run; csrc/rdf_math.h, rdf_plan.h, rdf_kernels.hip) and read
when the run ends; `rdf_normalise` turns counts into g_ab(r) and running coordination numbers, `rdf_tags` types and group labels
into the per-atom tags.  Used by every driver in examples/md with --rdf N.

`CorrelationRecorder` accumulates mean-square displacements and velocity autocorrelations per type along a run: a ring of the last
L frames lives on the device, and one C call per recorded frame (admp_md_tcf: csrc/tcf_math.h, tcf_plan.h, tcf_kernels.hip)
unwraps the frame in double, stores it and correlates it with every frame of the ring -- sums in double, fixed order, no float
atomics, nothing read back until the run ends.  `tcf_layout` sorts the counted atoms into single-type tiles, `tcf_normalise` turns
the sums into MSD(t) and VACF(t), `diffusion_einstein` and `diffusion_green_kubo` into self-diffusion coefficients, `vdos` into the
vibrational density of states.  Used by every driver in examples/md with --msd N.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._device import HipForceBase

KB = 0.0083144626          # kJ/mol/K
STREAM_LANGEVIN, STREAM_MAXWELL, STREAM_BAROSTAT = 0, 1, 2      # csrc/md_math.h: the users of the generator never share a counter
STREAM_VRESCALE = 3
BAR_PER_KJ_MOL_A3 = 16605.39      # 1 kJ/mol/A^3 in bar


def _checked(o, n_atoms, **tensors):
    """the library reads and writes raw pointers: anything but (n,3) contiguous tensors of the handle's precision on its
    device would be read or written out of bounds"""
    for name, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == o._device.index):
            raise ValueError('%s must be a tensor on the handle\'s device' % name)
        if t.dtype != o._dtype:
            raise ValueError('%s must be of the handle\'s precision (%s), got %s' % (name, o._dtype, t.dtype))
        if tuple(t.shape) != (n_atoms, 3):
            raise ValueError('%s must have shape (%d, 3), got %s' % (name, n_atoms, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)


class HarmonicBonded(HipForceBase):
    """E = sum_bonds k/2 (r - r0)^2 + sum_angles k/2 (theta - theta0)^2 with minimum-image vectors.
    bonds (nb, 2) int, bond_par (nb, 2) = (k, r0); angles (na, 3) int = (i, centre, k), angle_par (na, 2) = (k, theta0 / rad)."""

    def __init__(self, n_atoms, bonds, bond_par, angles, angle_par, device=None):
        super().__init__(n_atoms, None, None, None, device)

        def ints(x, w):
            a = np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1, w))
            return torch.as_tensor(a).to(self._device)
        self._bidx, self._aidx = ints(bonds, 2), ints(angles, 3)
        self._bpar = self._real(np.asarray(bond_par, dtype=np.float64).reshape(-1, 2))
        self._apar = self._real(np.asarray(angle_par, dtype=np.float64).reshape(-1, 2))
        if len(self._bidx) != len(self._bpar) or len(self._aidx) != len(self._apar):
            raise ValueError('index and parameter lists differ in length')
        for idx in (self._bidx, self._aidx):
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_atoms):
                raise ValueError('atom index out of range')
        self.energy_words = torch.zeros(2, dtype=torch.float64, device=self._device)      # (bonds, angles), accumulated

    def add_forces(self, positions, box, grad):
        """grad (Na,3 device tensor of the handle's precision) += dE/dpositions; the energies are added to `energy_words`
        (zero them with reset_energy(); read them with energy())."""
        self._use_current_stream()
        pos = self._real(positions, (self.n_atoms, 3))
        if not (isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype == self._dtype and grad.is_contiguous()):
            raise ValueError('grad must be a contiguous device tensor of the handle\'s precision')
        boxa, _ = self._harr('box', box, 9)
        P = self._ptr
        _lib.check(self._h, self._L.admp_md_bonded(self._h, P(pos), boxa, len(self._bidx), P(self._bidx), P(self._bpar),
                                                   len(self._aidx), P(self._aidx), P(self._apar), P(self.energy_words),
                                                   P(grad)), 'admp_md_bonded')
        return grad

    def reset_energy(self):
        self.energy_words.zero_()

    def energy(self):
        """(host read) sum of the accumulated words"""
        return float(self.energy_words.sum())

    def get_forces(self, positions, box):
        """(E, dE/dpositions) of one evaluation -- the calculators' convention (one host read)"""
        self.reset_energy()
        g = torch.zeros((self.n_atoms, 3), dtype=self._dtype, device=self._device)
        self.add_forces(positions, box, g)
        return np.float64(self.energy()), self._like(g, positions)

    def get_energy_and_box_gradient(self, positions, box):
        """(E, dE/dbox (3,3)) at fixed Cartesian positions -- the calculators' convention.  Only the bond and angle vectors
        that the minimum image translates by a lattice vector contribute: the kernel sums shift^T (x) dE/dd over them
        (admp_md_bonded_box), dE/dbox = box^-T S is formed here.  One launch, one host read; `energy_words` is not touched."""
        self._use_current_stream()
        pos = self._real(positions, (self.n_atoms, 3))
        h = np.array(box.detach().cpu().numpy() if isinstance(box, torch.Tensor) else box, dtype=np.float64).reshape(3, 3)
        boxa, _ = self._harr('box', h, 9)
        words = torch.zeros(11, dtype=torch.float64, device=self._device)      # (E bonds, E angles, S row-major)
        P = self._ptr
        _lib.check(self._h, self._L.admp_md_bonded_box(self._h, P(pos), boxa, len(self._bidx), P(self._bidx), P(self._bpar),
                                                       len(self._aidx), P(self._aidx), P(self._apar), P(words), P(words[2:])),
                   'admp_md_bonded_box')
        w = words.cpu().numpy()
        return np.float64(w[0] + w[1]), np.linalg.inv(h).T @ w[2:].reshape(3, 3)

    def get_box_gradient(self, positions, box):
        return self.get_energy_and_box_gradient(positions, box)[1]


class VelocityVerlet:
    """r, v in A and A/fs, gradients in kJ/mol/A, masses in amu: v -= (dt/2) 1e-4 grad / m; r += dt v (1 kJ/mol/A/amu = 1e-4
    A/fs^2).  Both arrays are updated in place by one kernel per half step (the handle of any calculator lends its stream)."""
    ACC = 1e-4

    def __init__(self, handle_owner, masses, dt_fs):
        self._o = handle_owner
        self.dt = float(dt_fs)
        self.inv_mass = (1.0 / handle_owner._real(np.asarray(masses, dtype=np.float64).reshape(-1))).contiguous()
        self.ekin_word = torch.zeros(1, dtype=torch.float64, device=handle_owner._device)

    def _call(self, pos, vel, grad, drift, want_ekin):
        o = self._o
        o._use_current_stream()
        if want_ekin:
            self.ekin_word.zero_()
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_kick_drift(o._h, vel.shape[0], P(pos), P(vel), P(grad), P(self.inv_mass),
                                                 0.5 * self.dt * self.ACC, self.dt if drift else 0.0,
                                                 P(self.ekin_word) if want_ekin else None), 'admp_md_kick_drift')

    def kick_drift(self, pos, vel, grad):
        """first half: v(t + dt/2), r(t + dt)"""
        self._call(pos, vel, grad, True, False)

    def kick(self, pos, vel, grad, want_ekin=False):
        """second half: v(t + dt); want_ekin: the kinetic energy (kJ/mol) of the new velocities lands in ekin_word"""
        self._call(pos, vel, grad, False, want_ekin)

    def kinetic_energy(self):
        """(host read) sum m v^2 / 2 of the last kick(want_ekin=True), in kJ/mol"""
        return float(self.ekin_word[0]) / self.ACC


def random_fill(handle_owner, kind, n, seed, step, stream):
    """The generator of csrc/md_math.h written to a new device tensor (admp_md_random): kind 0: (n,4) words as int32 bit
    patterns (torch has no arithmetic on uint32; view them with numpy), kind 1: (n,3) standard normals of the handle's
    precision.  Row i is a function of (seed, step, stream, i) alone."""
    o = handle_owner
    o._use_current_stream()
    n = int(n)
    if n < 0:
        raise ValueError('n must not be negative')
    out = torch.empty((n, 4), dtype=torch.int32, device=o._device) if kind == 0 else \
        torch.empty((n, 3), dtype=o._dtype, device=o._device)
    _lib.check(o._h, o._L.admp_md_random(o._h, int(kind), n, int(seed), int(step), int(stream), o._ptr(out)), 'admp_md_random')
    return out


def maxwell_boltzmann(handle_owner, masses, temperature, seed, remove_com=True):
    """(n,3) device velocities in A/fs at `temperature` (K) for `masses` (amu): the normals of (seed, step 0, stream 1) times
    sqrt(1e-4 kB T / m); remove_com: minus the mass-weighted mean velocity (the temperature is then the one over 3n - 3
    degrees of freedom)."""
    o = handle_owner
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    if temperature < 0 or not np.all(m > 0):
        raise ValueError('temperature must not be negative and masses must be positive')
    xi = random_fill(o, 1, len(m), seed, 0, STREAM_MAXWELL)
    vel = xi * o._real(np.sqrt(VelocityVerlet.ACC * KB * float(temperature) / m))[:, None]
    if remove_com:
        m64 = torch.as_tensor(m, device=o._device)
        vel -= ((m64[:, None] * vel.double()).sum(0) / m64.sum()).to(vel.dtype)
    return vel.contiguous()


class Langevin:
    """BAOAB Langevin dynamics at `temperature` (K) with friction `friction_per_fs` (1/fs); units as in VelocityVerlet.
    kick_drift is B, A, O, A in one kernel (v -= (dt/2) 1e-4 grad / m; r += (dt/2) v; v = c1 v + sqrt((1 - c1^2) 1e-4 kB T / m)
    xi, c1 = exp(-friction dt); r += (dt/2) v) with xi drawn from (seed, step, stream 0, atom); kick is the closing B
    (admp_md_kick_drift).  `step` counts the kick_drift calls and may be set (a restart draws the same noise again).
    friction 0 is velocity Verlet."""
    ACC = VelocityVerlet.ACC

    def __init__(self, handle_owner, masses, dt_fs, temperature, friction_per_fs, seed):
        self._o = handle_owner
        self.dt = float(dt_fs)
        self.T = float(temperature)
        self.friction = float(friction_per_fs)
        self.seed = int(seed)
        self.step = 0
        if self.T < 0 or self.friction < 0 or self.dt < 0 or not 0 <= self.seed < 2 ** 64:
            raise ValueError('temperature, friction and dt must not be negative; the seed is an unsigned 64-bit number')
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if not np.all(m > 0):
            raise ValueError('masses must be positive')
        self.n_atoms = len(m)
        self.inv_mass = handle_owner._real(1.0 / m)
        self.c1 = float(np.exp(-self.friction * self.dt))
        self.c2sq_kT_acc = (1.0 - self.c1 * self.c1) * KB * self.T * self.ACC
        self.ekin_word = torch.zeros(1, dtype=torch.float64, device=handle_owner._device)

    def _checked(self, **tensors):
        _checked(self._o, self.n_atoms, **tensors)

    def kick_drift(self, pos, vel, grad, want_ekin=False):
        """first half: r(t + dt) and the velocities after the friction step; then step += 1"""
        self._checked(pos=pos, vel=vel, grad=grad)
        o = self._o
        o._use_current_stream()
        if want_ekin:
            self.ekin_word.zero_()
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_langevin(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass),
                                               0.5 * self.dt * self.ACC, self.dt, self.c1, self.c2sq_kT_acc, self.seed,
                                               int(self.step) & (2 ** 64 - 1), P(self.ekin_word) if want_ekin else None),
                   'admp_md_langevin')
        self.step += 1

    def kick(self, pos, vel, grad, want_ekin=False):
        """second half: v(t + dt) with the gradient at r(t + dt); want_ekin: the kinetic energy of the new velocities lands
        in ekin_word"""
        self._checked(pos=pos, vel=vel, grad=grad)
        o = self._o
        o._use_current_stream()
        if want_ekin:
            self.ekin_word.zero_()
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_kick_drift(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass),
                                                 0.5 * self.dt * self.ACC, 0.0, P(self.ekin_word) if want_ekin else None),
                   'admp_md_kick_drift')

    def kinetic_energy(self):
        """(host read) sum m v^2 / 2 of the last call with want_ekin=True, in kJ/mol"""
        return float(self.ekin_word[0]) / self.ACC

    def temperature(self, n_dof=None):
        """(host read) 2 Ekin / (n_dof kB) of the last call with want_ekin=True; n_dof defaults to 3 N"""
        return 2.0 * self.kinetic_energy() / ((3 * self.n_atoms if n_dof is None else n_dof) * KB)


class MTSLangevin:
    """Impulse multiple time stepping with two levels (r-RESPA; OpenMM's MTSLangevinIntegrator): the bonded terms of `bonded`
    (a HarmonicBonded: it lends its handle, its lists and its energy words) advance by `n_inner` BAOAB steps of length
    dt_outer / n_inner inside one kernel (admp_md_mts_step), everything the calculators compute acts once per outer step:

        kick_drift:  v -= (dt_outer/2) 1e-4 grad_slow / m;  n_inner x [B A O A on the bonded terms, f at the new r, B]
        (the calculators: grad_slow at the new r, WITHOUT the bonded terms)
        kick:        v -= (dt_outer/2) 1e-4 grad_slow / m                                         (admp_md_kick_drift, dt = 0)

    Units as in VelocityVerlet; c1 = exp(-friction dt_outer / n_inner); the noise of inner step k of outer step s is that of
    (seed, s n_inner + k, stream 0, atom), so n_inner = 1 is `Langevin` on the summed gradient and friction 0 is NVE r-RESPA.
    `step` counts the kick_drift calls and may be set (a restart draws the same noise again).  The atoms are integrated in
    tiles of whole molecules (connected components of the lists) of at most `tile_atoms` atoms (None: the library's default);
    a larger molecule is refused with ValueError.  r and v do not depend on tile_atoms, bit for bit."""
    ACC = VelocityVerlet.ACC
    MAX_TILE_ATOMS = 256          # csrc/mts_plan.h kMtsMaxTileAtoms

    def __init__(self, bonded, masses, dt_outer_fs, n_inner, temperature=0.0, friction_per_fs=0.0, seed=0, tile_atoms=None):
        if not isinstance(bonded, HarmonicBonded):
            raise ValueError('bonded must be a HarmonicBonded')
        self._o = bonded
        self.dt = float(dt_outer_fs)
        self.n_inner = int(n_inner)
        self.T = float(temperature)
        self.friction = float(friction_per_fs)
        self.seed = int(seed)
        self.step = 0
        if self.T < 0 or self.friction < 0 or self.dt < 0 or not 0 <= self.seed < 2 ** 64:
            raise ValueError('temperature, friction and dt must not be negative; the seed is an unsigned 64-bit number')
        if self.n_inner < 1 or self.n_inner != n_inner:
            raise ValueError('n_inner must be an integer of at least 1')
        if tile_atoms is not None and not (tile_atoms == int(tile_atoms) and 1 <= tile_atoms <= self.MAX_TILE_ATOMS):
            raise ValueError('tile_atoms must be None or between 1 and %d' % self.MAX_TILE_ATOMS)
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if not np.all(m > 0):
            raise ValueError('masses must be positive')
        if len(m) != bonded.n_atoms:
            raise ValueError('%d masses for the %d atoms of bonded' % (len(m), bonded.n_atoms))
        self.n_atoms = len(m)
        self.inv_mass = bonded._real(1.0 / m)
        self.c1 = float(np.exp(-self.friction * self.dt / self.n_inner))
        self.c2sq_kT_acc = (1.0 - self.c1 * self.c1) * KB * self.T * self.ACC
        self.ekin_word = torch.zeros(1, dtype=torch.float64, device=bonded._device)
        self._tile_atoms = 0 if tile_atoms is None else int(tile_atoms)
        self._plan()

    def _plan(self):
        """the handle keeps one plan: made here, and again by kick_drift when another MTSLangevin on the same `bonded` has
        replaced it since"""
        bonded = self._o
        bidx = np.ascontiguousarray(bonded._bidx.cpu().numpy(), dtype=np.int32)
        aidx = np.ascontiguousarray(bonded._aidx.cpu().numpy(), dtype=np.int32)
        bpar = np.ascontiguousarray(bonded._bpar.cpu().numpy(), dtype=np.float64)
        apar = np.ascontiguousarray(bonded._apar.cpu().numpy(), dtype=np.float64)
        rc = bonded._L.admp_md_mts_plan(bonded._h, self.n_atoms, len(bidx), bidx.ctypes.data, bpar.ctypes.data, len(aidx),
                                        aidx.ctypes.data, apar.ctypes.data, self._tile_atoms)
        if rc == -1:                                                  # ADMP_E_ARG: the plan's refusal
            msg = bonded._L.admp_last_error(bonded._h)
            raise ValueError('admp_md_mts_plan: %s' % (msg.decode() if msg else ''))
        _lib.check(bonded._h, rc, 'admp_md_mts_plan')
        bonded._mts_planned_by = self

    def kick_drift(self, pos, vel, grad_slow, box, fast_grad=None):
        """first half of an outer step in one kernel: r(t + dt_outer) and the velocities short of the closing kick;
        bonded.energy_words += (E_bonds, E_angles) at the new positions; fast_grad (optional) = the bonded gradient there;
        then step += 1"""
        tensors = dict(pos=pos, vel=vel, grad_slow=grad_slow)
        if fast_grad is not None:
            tensors['fast_grad'] = fast_grad
        _checked(self._o, self.n_atoms, **tensors)
        o = self._o
        o._use_current_stream()
        if getattr(o, '_mts_planned_by', None) is not self:
            self._plan()
        boxa, _ = o._harr('box', box, 9)
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_mts_step(o._h, self.n_atoms, P(pos), P(vel), P(grad_slow), P(self.inv_mass), boxa,
                                               0.5 * self.dt * self.ACC, self.dt, self.n_inner, self.c1, self.c2sq_kT_acc,
                                               self.seed, int(self.step) & (2 ** 64 - 1), P(o.energy_words), P(fast_grad)),
                   'admp_md_mts_step')
        self.step += 1

    def kick(self, pos, vel, grad_slow, want_ekin=False):
        """closing half kick of the outer step with the calculators' gradient at r(t + dt_outer); want_ekin: the kinetic energy
        of the new velocities lands in ekin_word"""
        _checked(self._o, self.n_atoms, pos=pos, vel=vel, grad_slow=grad_slow)
        o = self._o
        o._use_current_stream()
        if want_ekin:
            self.ekin_word.zero_()
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_kick_drift(o._h, self.n_atoms, P(pos), P(vel), P(grad_slow), P(self.inv_mass),
                                                 0.5 * self.dt * self.ACC, 0.0, P(self.ekin_word) if want_ekin else None),
                   'admp_md_kick_drift')

    def kinetic_energy(self):
        """(host read) sum m v^2 / 2 of the last kick(want_ekin=True), in kJ/mol"""
        return float(self.ekin_word[0]) / self.ACC

    def temperature(self, n_dof=None):
        """(host read) 2 Ekin / (n_dof kB) of the last kick(want_ekin=True); n_dof defaults to 3 N"""
        return 2.0 * self.kinetic_energy() / ((3 * self.n_atoms if n_dof is None else n_dof) * KB)

    def plan_info(self):
        """what the library planned: tiles, tile capacity, largest component, atoms, bonds, angles, LDS bytes per workgroup,
        launches so far"""
        out = (ctypes.c_int64 * 8)()
        _lib.check(self._o._h, self._o._L.admp_md_mts_info(self._o._h, out), 'admp_md_mts_info')
        keys = ('tiles', 'tile_atoms', 'largest_component', 'atoms', 'bonds', 'angles', 'lds_bytes', 'launches')
        return dict(zip(keys, (int(x) for x in out)))


class Constraints(HipForceBase):
    """Pairwise distance constraints |x_j - x_i| = d (minimum-image vectors) with a handle of their own: pairs (nc, 2) int,
    lengths (nc) in A, masses (n_atoms) in amu.  The connected components of the list ("clusters": a rigid water with O-H, O-H
    and H-H is one) are solved iteratively, whole clusters resident in LDS, one lane sweeping a cluster's constraints in the
    caller's order (admp_md_con_plan, csrc/con_plan.h): results are bit-identical from run to run and for every `tile_atoms`
    (None: the library's default; a larger cluster is refused with ValueError, like every other flaw of the lists).

    `tolerance` is relative to d: a sweep stops when every | |p|^2 - d^2 | <= 2 tolerance d^2 (positions) or
    |s.(v_j - v_i)| dt <= tolerance d^2 (velocities); at most `max_sweeps` sweeps are made whatever happens, and a cluster
    that stops unconverged counts in `failures()`.  In single precision a tolerance below a few 1e-7 cannot be met once the
    solved displacement is added to the positions (eps |r| / d: 6e-8 x 30 A / 1 A); the value is passed on as it is, not
    clamped -- watch `failures()`."""
    MAX_TILE_ATOMS = 256          # csrc/con_plan.h kConMaxTileAtoms

    def __init__(self, n_atoms, pairs, lengths, masses, tolerance=1e-6, max_sweeps=500, tile_atoms=None, device=None):
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.float64).reshape(-1))
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if len(pairs) != len(lengths):
            raise ValueError('%d pairs for %d lengths' % (len(pairs), len(lengths)))
        if len(m) != int(n_atoms):
            raise ValueError('%d masses for %d atoms' % (len(m), int(n_atoms)))
        if not (np.all(m > 0) and np.all(np.isfinite(m))):
            raise ValueError('masses must be positive and finite')
        if not (np.isfinite(tolerance) and tolerance >= 0):
            raise ValueError('tolerance must be finite and not negative')
        if max_sweeps != int(max_sweeps) or max_sweeps < 1:
            raise ValueError('max_sweeps must be an integer of at least 1')
        if tile_atoms is not None and not (tile_atoms == int(tile_atoms) and 1 <= tile_atoms <= self.MAX_TILE_ATOMS):
            raise ValueError('tile_atoms must be None or between 1 and %d' % self.MAX_TILE_ATOMS)
        if pairs.size and (pairs.min() < -2 ** 31 or pairs.max() >= 2 ** 31):
            raise ValueError('atom index out of range')
        super().__init__(n_atoms, None, None, None, device)
        self.tolerance, self.max_sweeps = float(tolerance), int(max_sweeps)
        self.masses = m
        self.inv_mass = self._real(1.0 / m)
        self._pairs, self._lengths = pairs.astype(np.int32), lengths
        self._tile_atoms = 0 if tile_atoms is None else int(tile_atoms)
        self.counters = torch.zeros(2, dtype=torch.int32, device=self._device)      # (failed clusters, most sweeps of a cluster)
        rc = self._L.admp_md_con_plan(self._h, self.n_atoms, len(self._pairs), self._pairs.ctypes.data, self._lengths.ctypes.data,
                                      self._tile_atoms)
        if rc == -1:                                                  # ADMP_E_ARG: the plan's refusal
            msg = self._L.admp_last_error(self._h)
            raise ValueError('admp_md_con_plan: %s' % (msg.decode() if msg else ''))
        _lib.check(self._h, rc, 'admp_md_con_plan')

    @property
    def n_constraints(self):
        return len(self._pairs)

    def project_positions(self, pos, box, ref=None):
        """pos (in place) moved onto the constraints along the directions of `ref` (None: of pos itself): what a minimised or
        perturbed configuration needs before a run.  Unconstrained atoms are not changed; a cluster's centre of mass moves
        by rounding only."""
        tensors = dict(pos=pos) if ref is None else dict(pos=pos, ref=ref)
        _checked(self, self.n_atoms, **tensors)
        self._use_current_stream()
        boxa, _ = self._harr('box', box, 9)
        P = self._ptr
        _lib.check(self._h, self._L.admp_md_con_project(self._h, self.n_atoms, P(pos), P(pos if ref is None else ref),
                                                        P(self.inv_mass), boxa, self.tolerance, self.max_sweeps, P(self.counters)),
                   'admp_md_con_project')

    def project_velocities(self, pos, vel, box, dt_fs=1.0):
        """vel (in place) without its components along the constraints at pos: every |s.(v_j - v_i)| dt_fs <= tolerance d^2.
        A cluster's linear momentum changes by rounding only."""
        _checked(self, self.n_atoms, pos=pos, vel=vel)
        if not (np.isfinite(dt_fs) and dt_fs > 0):
            raise ValueError('dt_fs must be positive and finite')
        self._use_current_stream()
        boxa, _ = self._harr('box', box, 9)
        P = self._ptr
        _lib.check(self._h, self._L.admp_md_con_kick(self._h, self.n_atoms, P(pos), P(vel), None, P(self.inv_mass), boxa, 0.0,
                                                     float(dt_fs), self.tolerance, self.max_sweeps, None, P(self.counters)),
                   'admp_md_con_kick')

    def failures(self):
        """(host read) clusters that stopped unconverged since the last reset_failures(), summed over the calls"""
        return int(self.counters[0])

    def max_sweeps_seen(self):
        """(host read) the most sweeps any cluster made in a call since the last reset_failures()"""
        return int(self.counters[1])

    def reset_failures(self):
        self.counters.zero_()

    def plan_info(self):
        """what the library planned: tiles, tile capacity, largest cluster, atoms, constraints, clusters, LDS bytes per
        workgroup, launches so far; and the lanes of a workgroup"""
        out = (ctypes.c_int64 * 8)()
        _lib.check(self._h, self._L.admp_md_con_info(self._h, out), 'admp_md_con_info')
        keys = ('tiles', 'tile_atoms', 'largest_cluster', 'atoms', 'constraints', 'clusters', 'lds_bytes', 'launches')
        info = dict(zip(keys, (int(x) for x in out)))
        info['lanes'] = 64 if info['tile_atoms'] <= 64 else (128 if info['tile_atoms'] <= 128 else 256)
        return info


class ConstrainedLangevin:
    """Constrained BAOAB (the splitting of OpenMM's LangevinMiddleIntegrator) on the constraints of a `Constraints`, which lends
    its handle, masses, tolerance and failure counter; units as in VelocityVerlet:

        kick_drift:  v -= (dt/2) 1e-4 grad / m;  delta = (dt/2) v;  v = c1 v + sig xi;  delta += (dt/2) v;  SHAKE on delta;
                     v += (delta - delta_unconstrained) / dt;  r += delta                              (admp_md_con_step)
        (the calculators: grad at the new r)
        kick:        v -= (dt/2) 1e-4 grad / m;  RATTLE on v                                              (admp_md_con_kick)

    one kernel each.  c1 = exp(-friction dt), xi the normals of (seed, step, stream 0, atom) of csrc/md_math.h; `step` counts
    the kick_drift calls and may be set (a restart draws the same noise again).  friction 0 is RATTLE velocity Verlet.  The
    kinetic temperature counts 3 N - n_constraints degrees of freedom by default."""
    ACC = VelocityVerlet.ACC

    def __init__(self, constraints, dt_fs, temperature=0.0, friction_per_fs=0.0, seed=0):
        if not isinstance(constraints, Constraints):
            raise ValueError('constraints must be a Constraints')
        self._o = constraints
        self.dt = float(dt_fs)
        self.T = float(temperature)
        self.friction = float(friction_per_fs)
        self.seed = int(seed)
        self.step = 0
        if self.T < 0 or self.friction < 0 or not 0 <= self.seed < 2 ** 64:
            raise ValueError('temperature and friction must not be negative; the seed is an unsigned 64-bit number')
        if not (np.isfinite(self.dt) and self.dt > 0):
            raise ValueError('dt must be positive and finite')
        self.n_atoms = constraints.n_atoms
        self.inv_mass = constraints.inv_mass
        self.c1 = float(np.exp(-self.friction * self.dt))
        self.c2sq_kT_acc = (1.0 - self.c1 * self.c1) * KB * self.T * self.ACC
        self.ekin_word = torch.zeros(1, dtype=torch.float64, device=constraints._device)

    def kick_drift(self, pos, vel, grad, box):
        """first half: r(t + dt) on the constraints and the velocities short of the closing kick; then step += 1"""
        o = self._o
        _checked(o, self.n_atoms, pos=pos, vel=vel, grad=grad)
        o._use_current_stream()
        boxa, _ = o._harr('box', box, 9)
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_con_step(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass), boxa,
                                               0.5 * self.dt * self.ACC, self.dt, self.c1, self.c2sq_kT_acc, self.seed,
                                               int(self.step) & (2 ** 64 - 1), o.tolerance, o.max_sweeps, P(o.counters)),
                   'admp_md_con_step')
        self.step += 1

    def kick(self, pos, vel, grad, box, want_ekin=False):
        """second half: v(t + dt) with the gradient at r(t + dt), on the constraints; want_ekin: the kinetic energy of the new
        velocities lands in ekin_word"""
        o = self._o
        _checked(o, self.n_atoms, pos=pos, vel=vel, grad=grad)
        o._use_current_stream()
        if want_ekin:
            self.ekin_word.zero_()
        boxa, _ = o._harr('box', box, 9)
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_con_kick(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass), boxa,
                                               0.5 * self.dt * self.ACC, self.dt, o.tolerance, o.max_sweeps,
                                               P(self.ekin_word) if want_ekin else None, P(o.counters)), 'admp_md_con_kick')

    def kinetic_energy(self):
        """(host read) sum m v^2 / 2 of the last kick(want_ekin=True), in kJ/mol"""
        return float(self.ekin_word[0]) / self.ACC

    def temperature(self, n_dof=None):
        """(host read) 2 Ekin / (n_dof kB) of the last kick(want_ekin=True); n_dof defaults to 3 N - n_constraints"""
        n_dof = 3 * self.n_atoms - self._o.n_constraints if n_dof is None else n_dof
        return 2.0 * self.kinetic_energy() / (n_dof * KB)


class CRescaleBarostat:
    """Isotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020) at `temperature` (K) and
    `pressure_bar`, with relaxation time `tau_p_fs` and isothermal compressibility `compressibility_per_bar`; units as in
    VelocityVerlet, pressures in bar.  With eps = ln V, one application advances the cell by dt_p (the caller applies it every
    dt_p / dt steps, after the closing kick):

        d eps = (beta_T / tau_p) (P_inst - P0) dt_p + sqrt(2 kB T beta_T dt_p / (V tau_p)) xi,   mu = exp(d eps / 3)
        r <- mu r,  box <- mu box,  v <- v / mu

    xi is the first normal of (seed, step, stream 2, atom 0) of csrc/md_math.h; `step` counts the applications and may be set
    (a restart draws the same noise again).  P_inst = (2 K / 3 - dE/d eps) / V with dE/d eps = (sum_ab box_ab (dE/dbox)_ab +
    sum_i r_i . g_i) / 3: `get_box_gradient` of every calculator is dE/dbox at fixed Cartesian positions, so the positions'
    share is added here.  The caller sums dE/dbox over its calculators; the barostat does not know them."""
    ACC = VelocityVerlet.ACC

    def __init__(self, handle_owner, masses, dt_p_fs, temperature, pressure_bar, tau_p_fs, compressibility_per_bar, seed):
        self._o = handle_owner
        self.dt_p = float(dt_p_fs)
        self.T = float(temperature)
        self.P0 = float(pressure_bar)
        self.tau_p = float(tau_p_fs)
        self.beta_T = float(compressibility_per_bar)
        self.seed = int(seed)
        self.step = 0
        if self.T < 0 or self.beta_T < 0 or self.dt_p < 0 or not self.tau_p > 0 or not 0 <= self.seed < 2 ** 64:
            raise ValueError('temperature, compressibility and dt_p must not be negative; tau_p must be positive; the seed is an '
                             'unsigned 64-bit number')
        if not all(np.isfinite(x) for x in (self.dt_p, self.T, self.P0, self.tau_p, self.beta_T)):
            raise ValueError('the barostat\'s parameters must be finite')
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if not np.all(m > 0):
            raise ValueError('masses must be positive')
        self.n_atoms = len(m)
        self.inv_mass = handle_owner._real(1.0 / m)
        self._words = torch.zeros(21, dtype=torch.float64, device=handle_owner._device)

    def sums(self, pos, vel, grad):
        """(kin, rg, xi): kin (3,3) = sum m v (x) v in kJ/mol (its trace is twice the kinetic energy), rg (3,3) = sum r (x) g
        with g = +dE/dr in kJ/mol, xi the normal of this application.  One launch and one host read; sums in double."""
        _checked(self._o, self.n_atoms, pos=pos, vel=vel, grad=grad)
        o = self._o
        o._use_current_stream()
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_virial(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass), self.seed,
                                             int(self.step) & (2 ** 64 - 1), P(self._words)), 'admp_md_virial')
        w = self._words.cpu().numpy()
        return w[0:9].reshape(3, 3) / self.ACC, w[9:18].reshape(3, 3).copy(), float(w[18])

    @staticmethod
    def _cell(box):
        h = np.asarray(box, dtype=np.float64).reshape(3, 3)
        return h, abs(float(np.linalg.det(h)))

    def pressure(self, box, dEdbox_total, kin, rg):
        """(host) P_inst in bar: (2 K / 3 - dE/d eps) / V"""
        h, vol = self._cell(box)
        dE_deps = (float((h * np.asarray(dEdbox_total, dtype=np.float64)).sum()) + float(np.trace(rg))) / 3.0
        return (float(np.trace(kin)) / 3.0 - dE_deps) / vol * BAR_PER_KJ_MOL_A3

    def pressure_tensor(self, box, dEdbox_total, kin, rg):
        """(host) (kin - box^T dE/dbox - rg) / V in bar, for logging: a third of its trace is `pressure`.  On a triclinic cell
        the reference's k-point order and spread operators leave it unsymmetric."""
        h, vol = self._cell(box)
        return (np.asarray(kin) - h.T @ np.asarray(dEdbox_total, dtype=np.float64) - np.asarray(rg)) / vol * BAR_PER_KJ_MOL_A3

    def apply(self, pos, vel, box, p_inst, xi):
        """one application: d eps and mu on the host in double, positions and velocities rescaled by one kernel, `box` (a
        float64 ndarray) multiplied IN PLACE by mu; then step += 1.  Returns mu."""
        _checked(self._o, self.n_atoms, pos=pos, vel=vel)
        if not (isinstance(box, np.ndarray) and box.dtype == np.float64 and box.size == 9 and box.flags.writeable):
            raise ValueError('box must be a writeable float64 ndarray of 9 elements (it is scaled in place)')
        # (d eps and mu: MolecularCRescaleBarostat.apply repeats these lines -- change both, or singleton groups no longer
        # reduce to this class; tests/test_gpu_md_molecular_barostat.py holds the two to the same mu)
        _, vol = self._cell(box)
        kT_bar = KB * self.T * BAR_PER_KJ_MOL_A3 / vol                      # kB T / V in bar
        d_eps = self.beta_T / self.tau_p * (float(p_inst) - self.P0) * self.dt_p + \
            np.sqrt(2.0 * kT_bar * self.beta_T * self.dt_p / self.tau_p) * float(xi)
        mu = float(np.exp(d_eps / 3.0))
        if not (np.isfinite(mu) and mu > 0.0):
            raise ValueError('the scale factor is not finite (P_inst %r, xi %r)' % (p_inst, xi))
        o = self._o
        o._use_current_stream()
        _lib.check(o._h, o._L.admp_md_scale(o._h, self.n_atoms, o._ptr(pos), o._ptr(vel), mu), 'admp_md_scale')
        box *= mu
        self.step += 1
        return mu


def groups_of(n_atoms, bonded=None, constraints=None):
    """(n_atoms) int32 group labels: the connected components of the bond and angle lists of `bonded` (a HarmonicBonded) and / or
    the pairs of `constraints` (a Constraints); an atom in no item is a group of its own.  The label of a group is its smallest
    atom."""
    n_atoms = int(n_atoms)
    edges = []
    if bonded is not None:
        b, a = bonded._bidx.cpu().numpy().reshape(-1, 2), bonded._aidx.cpu().numpy().reshape(-1, 3)
        edges += [b, a[:, :2], a[:, 1:]]
    if constraints is not None:
        edges.append(np.asarray(constraints._pairs).reshape(-1, 2))
    for owner in (bonded, constraints):
        if owner is not None and owner.n_atoms != n_atoms:
            raise ValueError('%d atoms, but the lists are those of %d' % (n_atoms, owner.n_atoms))
    label = np.arange(n_atoms, dtype=np.int64)
    e = np.concatenate(edges).astype(np.int64) if edges else np.zeros((0, 2), dtype=np.int64)
    while len(e):                                                     # label propagation to the smallest atom, with pointer jumping
        lo = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], lo)
        np.minimum.at(new, e[:, 1], lo)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return label.astype(np.int32)


class MolecularCRescaleBarostat(CRescaleBarostat):
    """`CRescaleBarostat` with molecular (centre-of-mass) scaling: what a system with constraints needs, since scaling every
    atom would stretch every constrained distance by mu, and the atomic pressure counts the kinetic energy and the virial of
    constrained degrees of freedom.  `groups` (n_atoms) assigns every atom to exactly one group by an integer label >= 0 (see
    `groups_of`; a singleton is a group); an atom may be wrapped into the cell independently of its group, and groups are
    assumed smaller than half the cell.  With the anchor a of a group its lowest-numbered atom,

        d_i = min_image(r_i - r_a),  s_i = (r_i - r_a) - d_i  (the lattice translation the image applied; exactly zero if none)
        R_c = r_a + sum m_i d_i / M,  V_c = sum m_i v_i / M,  R_c(i) = R_c + s_i  (the centre's image that belongs to atom i)

    one application with factor mu (box -> mu box) is r_i += (mu - 1) R_c(i), v_i += (1/mu - 1) V_c: a group moves rigidly,
    atoms of a group in the same image receive bitwise the same displacement dr and all its atoms the same dv, so distances and
    relative velocities inside a group change by the one rounding of r + dr and v + dv only.
    mu - 1 and 1/mu - 1 are formed on the host in double with expm1.  The pressure is the molecular one:

        P = (2 K_com / 3 - dE/d eps) / V,  2 K_com = sum_c M_c |V_c|^2,
        dE/d eps = (sum_ab box_ab (dE/dbox)_ab + sum_i R_c(i) . g_i) / 3

    with dE/dbox what `get_box_gradient` of every calculator returns (fixed Cartesian positions).  d eps, the noise and `step`
    are exactly those of `CRescaleBarostat`; with all-singleton groups everything reduces to it.  The groups are handled in
    tiles of whole groups of at most `tile_atoms` atoms (None: the library's default; a larger group is refused with
    ValueError); r and v do not depend on tile_atoms, bit for bit.  The plan has a slot of its own on the handle: a
    `Constraints` can lend its handle to this class and to a `ConstrainedLangevin` at once."""
    MAX_TILE_ATOMS = 256          # csrc/mol_plan.h kMolMaxTileAtoms

    def __init__(self, handle_owner, masses, groups, dt_p_fs, temperature, pressure_bar, tau_p_fs, compressibility_per_bar, seed,
                 tile_atoms=None):
        super().__init__(handle_owner, masses, dt_p_fs, temperature, pressure_bar, tau_p_fs, compressibility_per_bar, seed)
        if tile_atoms is not None and not (tile_atoms == int(tile_atoms) and 1 <= tile_atoms <= self.MAX_TILE_ATOMS):
            raise ValueError('tile_atoms must be None or between 1 and %d' % self.MAX_TILE_ATOMS)
        g = np.asarray(groups)
        if g.ndim != 1 or len(g) != self.n_atoms:
            raise ValueError('%s group labels for %d atoms' % (g.shape, self.n_atoms))
        if not np.issubdtype(g.dtype, np.integer) or (g.size and (g.min() < -2 ** 31 or g.max() >= 2 ** 31)):
            raise ValueError('the group labels must be 32-bit integers')
        self._groups = np.ascontiguousarray(g, dtype=np.int32)
        self._tile_atoms = 0 if tile_atoms is None else int(tile_atoms)
        self._plan()

    def _plan(self):
        """the handle keeps one plan: made here, and again by sums / apply when another barostat on the same handle has replaced
        it since"""
        o = self._o
        rc = o._L.admp_md_mol_plan(o._h, self.n_atoms, self._groups.ctypes.data, self._tile_atoms)
        if rc == -1:                                                  # ADMP_E_ARG: the plan's refusal
            msg = o._L.admp_last_error(o._h)
            raise ValueError('admp_md_mol_plan: %s' % (msg.decode() if msg else ''))
        _lib.check(o._h, rc, 'admp_md_mol_plan')
        o._mol_planned_by = self

    def _ready(self):
        o = self._o
        o._use_current_stream()
        if getattr(o, '_mol_planned_by', None) is not self:
            self._plan()
        return o

    def sums(self, pos, vel, grad, box):
        """(kin, rg, xi): kin (3,3) = sum_c M_c V_c (x) V_c in kJ/mol (its trace is twice the kinetic energy of the centres), rg
        (3,3) = sum_i R_c(i) (x) g_i with g = +dE/dr in kJ/mol, xi the normal of this application.  One launch and one host
        read; sums in double."""
        _checked(self._o, self.n_atoms, pos=pos, vel=vel, grad=grad)
        o = self._ready()
        boxa, _ = o._harr('box', box, 9)
        P = o._ptr
        _lib.check(o._h, o._L.admp_md_mol_sums(o._h, self.n_atoms, P(pos), P(vel), P(grad), P(self.inv_mass), boxa, self.seed,
                                               int(self.step) & (2 ** 64 - 1), P(self._words)), 'admp_md_mol_sums')
        w = self._words.cpu().numpy()
        return w[0:9].reshape(3, 3) / self.ACC, w[9:18].reshape(3, 3).copy(), float(w[18])

    def apply(self, pos, vel, box, p_inst, xi):
        """one application: d eps on the host in double, mu - 1 and 1/mu - 1 by expm1, the groups moved by one kernel, `box` (a
        float64 ndarray) multiplied IN PLACE by mu; then step += 1.  Returns mu."""
        _checked(self._o, self.n_atoms, pos=pos, vel=vel)
        if not (isinstance(box, np.ndarray) and box.dtype == np.float64 and box.size == 9 and box.flags.writeable):
            raise ValueError('box must be a writeable float64 ndarray of 9 elements (it is scaled in place)')
        # (d eps and mu: the lines of CRescaleBarostat.apply, repeated because that class stays as it is and this one needs
        # d eps itself for expm1 -- change both)
        _, vol = self._cell(box)
        kT_bar = KB * self.T * BAR_PER_KJ_MOL_A3 / vol                      # kB T / V in bar
        d_eps = self.beta_T / self.tau_p * (float(p_inst) - self.P0) * self.dt_p + \
            np.sqrt(2.0 * kT_bar * self.beta_T * self.dt_p / self.tau_p) * float(xi)
        mu = float(np.exp(d_eps / 3.0))
        if not (np.isfinite(mu) and mu > 0.0):
            raise ValueError('the scale factor is not finite (P_inst %r, xi %r)' % (p_inst, xi))
        o = self._ready()
        boxa, _ = o._harr('box', box, 9)
        _lib.check(o._h, o._L.admp_md_mol_scale(o._h, self.n_atoms, o._ptr(pos), o._ptr(vel), o._ptr(self.inv_mass), boxa,
                                                float(np.expm1(d_eps / 3.0)), float(np.expm1(-d_eps / 3.0))), 'admp_md_mol_scale')
        box *= mu
        self.step += 1
        return mu

    def plan_info(self):
        """what the library planned: tiles, tile capacity, largest group, atoms, groups, LDS bytes per workgroup, lanes of a
        workgroup, launches so far"""
        out = (ctypes.c_int64 * 8)()
        _lib.check(self._o._h, self._o._L.admp_md_mol_info(self._o._h, out), 'admp_md_mol_info')
        keys = ('tiles', 'tile_atoms', 'largest_group', 'atoms', 'groups', 'lds_bytes', 'lanes', 'launches')
        return dict(zip(keys, (int(x) for x in out)))


class FireMinimizer:
    """FIRE energy minimiser (Bitzek et al., PRL 97, 170201, 2006) with the half step back of FIRE 2.0 (Guenole et al., Comput.
    Mater. Sci. 175, 109584, 2020), semi-implicit Euler and a hard displacement cap; units as in VelocityVerlet (the rule is
    csrc/md_fire_math.h, the entry admp_md_fire_step).  `masses` (amu; None: 1 for every atom) weigh the force step, w_i = 1e-4 /
    m_i.  Per iteration, with F = -grad, P = sum F.v:

        P > 0:      v <- (1 - alpha) v + alpha |v| F / |F| (norms over all atoms); after `n_delay` such steps in a row
                    dt <- min(dt f_inc, dt_max), alpha <- alpha f_alpha
        otherwise:  x <- x - (last step / 2) v;  v <- 0;  dt <- dt f_dec (not below dt_min);  alpha <- alpha_start
        then        v <- v + s w F;  x <- x + s v,   s the largest value <= dt for which no atom moves more than `max_step` (A)

    The minimiser owns the velocities `vel` and the state (2 x 8 doubles on the device: dt, alpha, n_pos, dtv_last, fmax,
    iterations, uphill steps, flags); `step` is one C call that reads nothing back, `info()` is one host read.  With
    `constraints` (a Constraints of the same atoms) every step is followed by the projection of positions and velocities onto
    them, so the minimum found is the one ON the constraints.  For a given number of atoms the result is a function of the
    inputs alone, bit for bit."""
    ACC = VelocityVerlet.ACC
    STATE_WORDS = ('dt', 'alpha', 'n_pos', 'dtv_last', 'fmax', 'iterations', 'uphill_steps')      # and the flags word
    DONE, FAILED = 1, 2

    def __init__(self, handle_owner, n_atoms, masses=None, *, dt_start_fs=0.5, dt_max_fs=5.0, dt_min_fs=0.01, max_step=0.1,
                 n_delay=20, f_inc=1.1, f_dec=0.5, alpha_start=0.25, f_alpha=0.99, constraints=None):
        self._o = handle_owner
        self.n_atoms = int(n_atoms)
        if self.n_atoms < 0 or self.n_atoms != n_atoms:
            raise ValueError('n_atoms must be an integer that is not negative')
        m = np.ones(self.n_atoms) if masses is None else np.asarray(masses, dtype=np.float64).reshape(-1)
        if len(m) != self.n_atoms:
            raise ValueError('%d masses for %d atoms' % (len(m), self.n_atoms))
        if not (np.all(m > 0) and np.all(np.isfinite(m))):
            raise ValueError('masses must be positive and finite')
        self.dt_start, self.dt_max, self.dt_min, self.max_step = float(dt_start_fs), float(dt_max_fs), float(dt_min_fs), float(max_step)
        self.n_delay, self.f_inc, self.f_dec = n_delay, float(f_inc), float(f_dec)
        self.alpha_start, self.f_alpha = float(alpha_start), float(f_alpha)
        for name in ('dt_start', 'dt_max', 'dt_min', 'max_step'):
            if not (np.isfinite(getattr(self, name)) and getattr(self, name) > 0):
                raise ValueError('%s must be positive and finite' % name)
        if not self.dt_min <= self.dt_start <= self.dt_max:
            raise ValueError('dt_min <= dt_start <= dt_max is required')
        if n_delay != int(n_delay) or n_delay < 0:
            raise ValueError('n_delay must be an integer that is not negative')
        if not (np.isfinite(self.f_inc) and self.f_inc >= 1):
            raise ValueError('f_inc must be finite and at least 1')
        for name in ('f_dec', 'alpha_start', 'f_alpha'):
            if not 0 < getattr(self, name) <= 1:
                raise ValueError('%s must lie in (0, 1]' % name)
        if constraints is not None and not (isinstance(constraints, Constraints) and constraints.n_atoms == self.n_atoms):
            raise ValueError('constraints must be a Constraints of the same %d atoms' % self.n_atoms)
        self.constraints = constraints
        self.inv_mass = handle_owner._real(1.0 / m)
        self._params = _lib.darr([self.dt_start, self.dt_max, self.dt_min, self.max_step, float(int(n_delay)), self.f_inc, self.f_dec,
                                  self.alpha_start, self.f_alpha])
        self.vel = torch.zeros((self.n_atoms, 3), dtype=handle_owner._dtype, device=handle_owner._device)
        self.state = torch.zeros((2, 8), dtype=torch.float64, device=handle_owner._device)
        self.reset()

    def reset(self):
        """velocities zero, a fresh state in both slots, call = 0: also what clears `failed`"""
        self.vel.zero_()
        fresh = torch.tensor([self.dt_start, self.alpha_start, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
        self.state.copy_(fresh.expand(2, 8))
        self.call = 0

    def step(self, pos, grad, ftol=0.0, box=None):
        """one iteration in place on pos and self.vel with grad = +dE/dpos at pos; nothing is read back.  Frozen (nothing moves)
        once max |F_i| <= ftol (`done`; a later call with a larger force resumes) or after a non-finite word (`failed`, until
        reset()).  box: the cell of the constraints, required with them."""
        o = self._o
        _checked(o, self.n_atoms, pos=pos, grad=grad)
        ftol = float(ftol)
        if not (np.isfinite(ftol) and ftol >= 0):
            raise ValueError('ftol must be finite and not negative')
        if self.constraints is not None and box is None:
            raise ValueError('box is required with constraints')
        o._use_current_stream()
        P = o._ptr
        rc = o._L.admp_md_fire_step(o._h, self.n_atoms, P(pos), P(self.vel), P(grad), P(self.inv_mass), self._params, ftol,
                                    self.call & (2 ** 64 - 1), P(self.state))
        if rc == -1:                                                  # ADMP_E_ARG
            msg = o._L.admp_last_error(o._h)
            raise ValueError('admp_md_fire_step: %s' % (msg.decode() if msg else ''))
        _lib.check(o._h, rc, 'admp_md_fire_step')
        self.call += 1
        if self.constraints is not None:
            self.constraints.project_positions(pos, box)
            self.constraints.project_velocities(pos, self.vel, box, dt_fs=self.dt_max)

    def info(self):
        """(host read) the state after the last step: dt, alpha, n_pos, dtv_last, fmax (the largest |F_i| the last step saw),
        iterations, uphill_steps, and the flags as the bools done and failed"""
        w = self.state[self.call & 1].cpu().numpy()
        out = dict(zip(self.STATE_WORDS, (float(x) for x in w[:7])))
        for k in ('n_pos', 'iterations', 'uphill_steps'):
            out[k] = int(out[k])
        out['done'], out['failed'] = int(w[7]) == self.DONE, int(w[7]) == self.FAILED
        return out

    def fmax(self):
        """(host read) the largest |F_i| the last step saw"""
        return self.info()['fmax']

    def converged(self):
        """(host read) whether the last step found max |F_i| <= ftol"""
        return self.info()['done']

    def minimize(self, pos, gradient_fn, ftol, max_iter, check_every=10, box=None):
        """at most max_iter iterations of grad = gradient_fn(pos); step(pos, grad, ftol, box), with one host read every
        `check_every` of them: stops on done, raises FloatingPointError on failed.  Returns info()."""
        if check_every != int(check_every) or check_every < 1:
            raise ValueError('check_every must be an integer of at least 1')
        for it in range(int(max_iter)):
            self.step(pos, gradient_fn(pos), ftol, box)
            if (it + 1) % check_every == 0:
                info = self.info()
                if info['failed']:
                    raise FloatingPointError('FIRE: a force or a velocity is not finite (iteration %d)' % info['iterations'])
                if info['done']:
                    return info
        info = self.info()
        if info['failed']:
            raise FloatingPointError('FIRE: a force or a velocity is not finite (iteration %d)' % info['iterations'])
        return info


class VRescale:
    """Stochastic velocity rescaling at `temperature` (K) with relaxation time `tau_fs` (Bussi, Donadio, Parrinello, J. Chem.
    Phys. 126, 014101, 2007); units as in VelocityVerlet (the rule is csrc/md_vrescale_math.h, the entry admp_md_vrescale).
    Once per step all velocities are multiplied by one factor alpha = sqrt(K' / K), where K is their kinetic energy and

        K' = (sqrt(c K) + sqrt((1 - c) kT / 2) R1)^2 + (1 - c) (kT / 2) S,   c = exp(-dt / tau), R1 ~ N(0, 1), S ~ chi^2(n_dof - 1)

    with R1 and S functions of (seed, step) alone (stream 3 of the generator).  `n_dof` defaults to 3 N; pass 3 N - n_constraints
    for constrained atoms, 3 N - 3 after maxwell_boltzmann(remove_com=True).  tau_fs = inf is c = 1 (alpha = 1 exactly: plain
    dynamics), tau_fs = 0 is c = 0 (a fresh canonical kinetic energy every step).

    `kick` is the closing half kick of a step (that of VelocityVerlet.kick or Langevin.kick, bit for bit) and the thermostat in
    one C call; `apply` is the thermostat alone, for after ConstrainedLangevin.kick, MTSLangevin.kick or a barostat's apply at
    friction 0.  Both then add 1 to `step`, which may be set (a restart draws the same noise again); `call` selects the slot of
    the state and is the object's own.  The state is 2 x 8 doubles on the device (K before, K after, alpha, heat, applications,
    tries, 0, flags); neither call reads anything back, `info()` is one host read.  E_pot + kinetic_energy() - heat() is the
    conserved quantity of the thermostatted dynamics.  A kinetic energy that is not finite sets `failed`: nothing is scaled from
    then on, until reset().  For a given number of atoms the result is a function of the inputs alone, bit for bit."""
    ACC = VelocityVerlet.ACC
    STATE_WORDS = ('k_before', 'k_after', 'alpha', 'heat', 'applications', 'tries')      # then a reserved word and the flags
    FAILED = 1

    def __init__(self, handle_owner, masses, dt_fs, temperature, tau_fs, seed, n_dof=None):
        self._o = handle_owner
        self.dt, self.T, self.tau, self.seed = float(dt_fs), float(temperature), float(tau_fs), int(seed)
        if not (np.isfinite(self.T) and self.T >= 0 and np.isfinite(self.dt) and self.dt >= 0 and self.tau >= 0
                and 0 <= self.seed < 2 ** 64):
            raise ValueError('temperature, tau and dt must not be negative (temperature and dt finite); the seed is an unsigned '
                             '64-bit number')
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if not (np.all(m > 0) and np.all(np.isfinite(m))):
            raise ValueError('masses must be positive and finite')
        self.n_atoms = len(m)
        self.n_dof = 3 * self.n_atoms if n_dof is None else n_dof
        if self.n_dof != int(self.n_dof) or self.n_dof < 1:
            raise ValueError('n_dof must be an integer of at least 1')
        self.n_dof = int(self.n_dof)
        self.c = 0.0 if self.tau == 0.0 else float(np.exp(-self.dt / self.tau))      # (tau = inf: 1)
        self.kT_acc = KB * self.T * self.ACC
        self.inv_mass = handle_owner._real(1.0 / m)
        self.state = torch.zeros((2, 8), dtype=torch.float64, device=handle_owner._device)
        self.step = 0
        self.reset()

    def reset(self):
        """a fresh state in both slots (alpha 1, everything else 0), call = 0: also what clears `failed`; `step` stays"""
        fresh = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
        self.state.copy_(fresh.expand(2, 8))
        self.call = 0

    def _apply(self, vel, grad):
        o = self._o
        o._use_current_stream()
        P = o._ptr
        rc = o._L.admp_md_vrescale(o._h, self.n_atoms, P(vel), None if grad is None else P(grad), P(self.inv_mass),
                                   0.5 * self.dt * self.ACC, self.n_dof, self.kT_acc, self.c, self.seed,
                                   int(self.step) & (2 ** 64 - 1), self.call & (2 ** 64 - 1), P(self.state))
        if rc == -1:                                                  # ADMP_E_ARG
            msg = o._L.admp_last_error(o._h)
            raise ValueError('admp_md_vrescale: %s' % (msg.decode() if msg else ''))
        _lib.check(o._h, rc, 'admp_md_vrescale')
        self.call += 1
        self.step += 1

    def kick(self, vel, grad):
        """second half of a step, v -= (dt/2) 1e-4 grad / m with the gradient at r(t + dt), then the thermostat; step += 1"""
        _checked(self._o, self.n_atoms, vel=vel, grad=grad)
        self._apply(vel, grad)

    def apply(self, vel):
        """the thermostat alone on the velocities as they are; step += 1"""
        _checked(self._o, self.n_atoms, vel=vel)
        self._apply(vel, None)

    def info(self):
        """(host read) the state after the last application: k_before, k_after, heat (kJ/mol), alpha, applications, tries (of
        the gamma deviate's rejection loop in the last draw), and the flag as the bool failed"""
        w = self.state[self.call & 1].cpu().numpy()
        out = dict(zip(self.STATE_WORDS, (float(x) for x in w[:6])))
        for k in ('k_before', 'k_after', 'heat'):
            out[k] /= self.ACC
        for k in ('applications', 'tries'):
            out[k] = int(out[k])
        out['failed'] = int(w[7]) == self.FAILED
        return out

    def kinetic_energy(self):
        """(host read) sum m v^2 / 2 of the velocities the last application left, in kJ/mol"""
        return self.info()['k_after']

    def temperature(self):
        """(host read) 2 Ekin / (n_dof kB) of the velocities the last application left"""
        return 2.0 * self.kinetic_energy() / (self.n_dof * KB)

    def heat(self):
        """(host read) the accumulated sum of (K after - K before) over the applications since reset(), in kJ/mol"""
        return self.info()['heat']


# ---- the dipole observable (include/admp_hip.h admp_pme_dipoles; csrc/dipole_math.h) ------------------------------------------
DEBYE_PER_E_ANGSTROM = 4.80320471


def group_csr(groups):
    """group labels (n_atoms; see `groups_of`) -> (group_start (n_groups + 1), group_atoms (n_atoms)), int32: the groups
    ordered by their smallest atom, the atoms ascending inside a group, so that a group's anchor comes first."""
    g = np.asarray(groups)
    if g.ndim != 1:
        raise ValueError('the group labels must be one-dimensional, got shape %s' % (g.shape,))
    if g.size and not np.issubdtype(g.dtype, np.integer):
        raise ValueError('the group labels must be integers')
    n = len(g)
    if n >= 2 ** 31:
        raise ValueError('too many atoms')
    _, inv = np.unique(g, return_inverse=True)
    inv = inv.reshape(-1)
    n_groups = int(inv.max()) + 1 if n else 0
    first = np.full(n_groups, n, dtype=np.int64)
    np.minimum.at(first, inv, np.arange(n))
    rank = np.empty(n_groups, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(n_groups)
    gid = rank[inv]                                                   # the group of every atom, groups by smallest atom
    atoms = np.argsort(gid, kind='stable')                            # (stable: ascending inside a group)
    start = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=n_groups))])
    return start.astype(np.int32), atoms.astype(np.int32)


def _checked_as(o, shape, **tensors):
    """`_checked` for any shape"""
    for name, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == o._device.index):
            raise ValueError('%s must be a tensor on the handle\'s device' % name)
        if t.dtype != o._dtype:
            raise ValueError('%s must be of the handle\'s precision (%s), got %s' % (name, o._dtype, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)


class _DipoleInputs:
    """what a dipole call needs besides the step's arrays, on the device of `pme`: the CSR pair of the groups and 1 / m.  Made
    once per (labels, masses) and kept on the calculator, so that neither is marshalled again step after step."""

    def __init__(self, pme, groups, masses):
        n = pme.n_atoms
        g = np.asarray(groups)
        if g.ndim != 1 or len(g) != n:
            raise ValueError('%s group labels for %d atoms' % (g.shape, n))
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        if len(m) != n:
            raise ValueError('%d masses for %d atoms' % (len(m), n))
        if not (np.all(m > 0) and np.all(np.isfinite(m))):
            raise ValueError('masses must be positive and finite')
        start, atoms = group_csr(g)
        self.n_groups = len(start) - 1
        self.start = torch.as_tensor(start).to(pme._device)
        self.atoms = torch.as_tensor(atoms).to(pme._device)
        self.inv_mass = pme._real(1.0 / m)

    @classmethod
    def of(cls, pme, groups, masses):
        g = np.ascontiguousarray(np.asarray(groups))
        m = np.ascontiguousarray(np.asarray(masses, dtype=np.float64))
        key = (g.dtype.str, g.shape, g.tobytes(), m.tobytes())
        cache = pme.__dict__.setdefault('_dipole_inputs', {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 4:
                cache.clear()
            hit = cache[key] = cls(pme, g, m)
        return hit


def _dipoles_into(pme, inp, positions, box, Q_local, U, mu, out16_ptr):
    """one admp_pme_dipoles call on the current stream: the arguments checked (the library reads raw pointers), the 16 words
    written at `out16_ptr`, the molecular dipoles into `mu` (a device tensor, or None).  No host read."""
    n = pme.n_atoms
    _checked_as(pme, (n, 3), positions=positions)
    _checked_as(pme, (n, 9), Q_local=Q_local)
    if U is None and pme.lpol:
        if not getattr(pme, '_have_U', False):
            raise RuntimeError('U=None on a polarizable calculator means the dipoles of its last get_forces / get_energy call, '
                               'and there has been none')
        U = pme._real(pme.U_ind, (n, 3))
    elif U is not None:
        _checked_as(pme, (n, 3), U=U)
    pme._use_current_stream()
    boxa, _ = pme._harr('box', box, 9)
    P = pme._ptr
    rc = pme._L.admp_pme_dipoles(pme._h, P(positions), boxa, P(Q_local), P(U), P(inp.inv_mass), inp.n_groups, P(inp.start),
                                 P(inp.atoms), P(mu), out16_ptr)
    if rc == _lib.E_ARG:
        msg = pme._L.admp_last_error(pme._h)
        raise ValueError('admp_pme_dipoles: %s' % (msg.decode() if msg else ''))
    _lib.check(pme._h, rc, 'admp_pme_dipoles')


def _dipole_dict(w, mu=None):
    """the 16 words of admp_pme_dipoles (host) as the dict of ADMPPmeForce.get_dipoles"""
    ng = max(float(w[12]), 1.0)
    out = {'M_charge': w[0:3].copy(), 'M_permanent': w[3:6].copy(), 'M_induced': w[6:9].copy(), 'mean_abs': float(w[9] / ng),
           'rms': float(np.sqrt(w[10] / ng)), 'max_abs': float(w[11])}
    out['M'] = out['M_charge'] + out['M_permanent'] + out['M_induced']
    if mu is not None:
        out['mu'] = mu
    return out


class DipoleRecorder:
    """Records the dipole observable along a run without a host read per step.  `pme` is the ADMPPmeForce whose topology defines
    the frames, `groups` the labels of `groups_of` (molecules), `masses` in any unit.  `record` writes the 16 words of
    admp_pme_dipoles (include/admp_hip.h: the charge, permanent and induced parts of the cell dipole M, sum |mu_c|, sum |mu_c|^2,
    max |mu_c|, the number of groups; e A) into the next row of a device array of `n_rows` rows; `rows()` is the one host read."""

    def __init__(self, pme, groups, masses, n_rows):
        if int(n_rows) != n_rows or n_rows < 0:
            raise ValueError('n_rows must be a non-negative integer')
        self._pme = pme
        self._inp = _DipoleInputs.of(pme, groups, masses)
        self.n_rows = int(n_rows)
        self._rows = torch.zeros((self.n_rows, 16), dtype=torch.float64, device=pme._device)
        self.k = 0

    def record(self, positions, box, Q_local, U=None):
        """row k of the array from the arrays of this step (device tensors of the calculator's precision; U=None on a
        polarizable calculator: the dipoles of its last get_forces call), then k += 1.  IndexError when the array is full."""
        if self.k >= self.n_rows:
            raise IndexError('the recorder\'s %d rows are full' % self.n_rows)
        _dipoles_into(self._pme, self._inp, positions, box, Q_local, U, None, self._rows.data_ptr() + 128 * self.k)
        self.k += 1

    def rows(self):
        """(host read) the rows recorded so far, (k, 16) float64"""
        return self._rows[:self.k].cpu().numpy()

    def summary(self):
        """(host read) the list of `get_dipoles`-style dicts of the rows recorded so far"""
        return [_dipole_dict(w) for w in self.rows()]

    def reset(self):
        """start over at row 0"""
        self.k = 0


def dielectric_constant(M_rows, volume, temperature):
    """static dielectric constant from the fluctuations of the cell dipole (conducting boundary, as Ewald sums imply):
    1 + 4 pi DIELECTRIC (<M . M> - <M> . <M>) / (3 V kB T), with M_rows (n, 3) in e A, the volume in A^3, the temperature in K
    and DIELECTRIC = e^2 / (4 pi eps0) in kJ/mol A of admp_amd.pme.  Pure numpy."""
    from .pme import DIELECTRIC
    M = np.asarray(M_rows, dtype=np.float64).reshape(-1, 3)
    if len(M) == 0:
        raise ValueError('no rows')
    mean = M.mean(axis=0)
    fluct = (M * M).sum(axis=1).mean() - mean @ mean
    return 1.0 + 4.0 * np.pi * DIELECTRIC * fluct / (3.0 * float(volume) * KB * float(temperature))


# ---- radial distribution functions (include/admp_hip.h admp_md_rdf; csrc/rdf_math.h, rdf_plan.h) ------------------------------
RDF_MAX_TYPES, RDF_MAX_COUNTERS, RDF_NOT_COUNTED, RDF_MAX_GROUPS = 8, 16384, 15, 2 ** 27
RDF_FORMS = ('none', 'tiles', 'cells')      # info()['form']: word 0 of admp_md_rdf's info4


def rdf_channel(a, b, n_types):
    """the row of the unordered type pair (a, b) in the histogram (csrc/rdf_math.h rdf_channel)"""
    a, b = (a, b) if a <= b else (b, a)
    return a * n_types - a * (a - 1) // 2 + (b - a)


def rdf_tags(types, groups=None):
    """per-atom types (ints; negative: not counted; at most 0..7) and group labels (those of `groups_of`; None: every atom its
    own group, no exclusions) -> (tags int32 = type | group << 4 as admp_md_rdf reads them, n_types, atoms per type)"""
    t = np.asarray(types)
    if t.ndim != 1 or (t.size and not np.issubdtype(t.dtype, np.integer)):
        raise ValueError('types must be a one-dimensional array of integers')
    n = len(t)
    t = t.astype(np.int64)
    if n and t.max() >= RDF_MAX_TYPES:
        raise ValueError('at most %d types (0..%d), got type %d' % (RDF_MAX_TYPES, RDF_MAX_TYPES - 1, t.max()))
    n_types = max(int(t.max()) + 1, 1) if n else 1
    if groups is None:
        g = np.arange(n, dtype=np.int64)
    else:
        g = np.asarray(groups)
        if g.ndim != 1 or len(g) != n or (g.size and not np.issubdtype(g.dtype, np.integer)):
            raise ValueError('groups must be %d integer labels, got shape %s' % (n, g.shape))
        g = np.unique(g, return_inverse=True)[1].reshape(-1).astype(np.int64)
    if n and g.max() >= RDF_MAX_GROUPS:
        raise ValueError('at most 2^27 groups')
    tags = (np.where(t < 0, RDF_NOT_COUNTED, t) | (g << 4)).astype(np.int32)
    return tags, n_types, np.bincount(t[t >= 0], minlength=n_types).astype(np.int64)


def rdf_normalise(counts, type_counts, r_max, n_frames, sum_inv_volume):
    """pair counts -> (r, g, n).  counts (channels, n_bins): the pairs per channel (rdf_channel) and bin summed over n_frames
    frames, type_counts the atoms N_a of every type, sum_inv_volume the sum of 1 / V over the frames.  r: the bin centres;
    g[(a, b)] = g[(b, a)] = counts / (N_pairs V_shell sum 1/V) with V_shell = 4 pi / 3 (r_{k+1}^3 - r_k^3) and N_pairs = N_a N_b
    (a != b) or N_a (N_a - 1) / 2 (a = b): exact for an ideal gas, also under a changing cell; n[(a, b)] the running coordination
    number of b around a at the upper edge of every bin, counts summed up over (N_a n_frames), twice that for a = b (a pair is
    counted once and belongs to both).  Channels without pairs give zeros.  Pure numpy."""
    c = np.asarray(counts).astype(np.float64)
    N = np.asarray(type_counts, dtype=np.float64).reshape(-1)
    n_types = len(N)
    if c.ndim != 2 or c.shape[0] != n_types * (n_types + 1) // 2:
        raise ValueError('counts must be (channels, n_bins) with %d channels, got %s' % (n_types * (n_types + 1) // 2, c.shape))
    n_bins = c.shape[1]
    edges = np.arange(n_bins + 1) * (float(r_max) / n_bins)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    r = 0.5 * (edges[1:] + edges[:-1])
    g, cn = {}, {}
    for a in range(n_types):
        for b in range(a, n_types):
            row = c[rdf_channel(a, b, n_types)]
            pairs = N[a] * N[b] if a != b else 0.5 * N[a] * (N[a] - 1.0)
            norm = pairs * shell * float(sum_inv_volume)
            g[(a, b)] = g[(b, a)] = row / norm if pairs > 0 and sum_inv_volume > 0 else np.zeros(n_bins)
            cum = np.cumsum(row)
            for x, y in ((a, b), (b, a)):
                cn[(x, y)] = (2.0 if a == b else 1.0) * cum / (N[x] * n_frames) if N[x] > 0 and n_frames > 0 else np.zeros(n_bins)
    return r, g, cn


class RdfRecorder:
    """Accumulates the typed pair-distance histogram of a run on the device: g_ab(r) and the coordination numbers without a host
    read per frame.  `handle_owner` is any object with a handle (a calculator, a HarmonicBonded); no topology and no pair list are
    needed.  `types` (ints, negative: not counted, at most 8 types) and `groups` (the labels of `groups_of`: pairs inside a group
    are not counted; None: no exclusions) are fixed at construction; `r_max` (at most half of every perpendicular height of every
    cell recorded) and `n_bins` fix the bins, channels x n_bins <= 16384.  `record` is one C call (admp_md_rdf) that adds the
    frame's counts with integer atomics, so the counts are the same bit for bit from run to run; `counts()` is the one host read;
    `force` (0 auto, 1 tiles, 2 cells) selects the kernel for tests and measurements."""

    def __init__(self, handle_owner, types, r_max, n_bins, groups=None):
        self._o = handle_owner
        tags, self.n_types, self.type_counts = rdf_tags(types, groups)
        self.n_atoms = len(tags)
        self.channels = self.n_types * (self.n_types + 1) // 2
        if int(n_bins) != n_bins or n_bins < 1:
            raise ValueError('n_bins must be a positive integer')
        self.n_bins, self.r_max = int(n_bins), float(r_max)
        if not (np.isfinite(self.r_max) and self.r_max > 0):
            raise ValueError('r_max must be positive and finite')
        if self.channels * self.n_bins > RDF_MAX_COUNTERS:
            raise ValueError('%d channels x %d bins exceed %d counters' % (self.channels, self.n_bins, RDF_MAX_COUNTERS))
        self._tags = torch.as_tensor(tags).to(handle_owner._device)
        self._hist = torch.zeros(self.channels * self.n_bins, dtype=torch.int64, device=handle_owner._device)
        self._info = (ctypes.c_int64 * 4)()
        self.force = 0
        self.frames, self.sum_inv_volume = 0, 0.0

    def record(self, positions, box):
        """adds the frame's counts (positions: an (n, 3) device tensor of the handle's precision; box: 9 host values, rows) and
        1 / V on the host; no host read.  ValueError for what the library refuses as an argument (r_max above half a height of
        this cell, a singular box): nothing is counted then."""
        o = self._o
        _checked_as(o, (self.n_atoms, 3), positions=positions)
        boxa, _ = o._harr('rdf_box', box, 9)
        o._use_current_stream()
        P = o._ptr
        rc = o._L.admp_md_rdf(o._h, self.n_atoms, P(positions), boxa, P(self._tags), self.n_types, self.r_max, self.n_bins,
                              P(self._hist), int(self.force), self._info)
        if rc == _lib.E_ARG:
            msg = o._L.admp_last_error(o._h)
            raise ValueError('admp_md_rdf: %s' % (msg.decode() if msg else ''))
        _lib.check(o._h, rc, 'admp_md_rdf')
        h = np.frombuffer(boxa, dtype=np.float64).reshape(3, 3)
        self.sum_inv_volume += 1.0 / abs(float(np.linalg.det(h)))
        self.frames += 1

    def counts(self):
        """(host read) the pair counts so far, (channels, n_bins) uint64; row rdf_channel(a, b, n_types) is the type pair (a, b)"""
        return self._hist.cpu().numpy().view(np.uint64).reshape(self.channels, self.n_bins)

    def reset(self):
        """zero counts (a memset on the current stream), no frames"""
        self._hist.zero_()
        self.frames, self.sum_inv_volume = 0, 0.0

    def info(self):
        """what the last record launched: form ('none', 'tiles', 'cells'), workgroups, tiles or cells, LDS bytes of a workgroup"""
        w = [int(x) for x in self._info]
        return {'form': RDF_FORMS[w[0]], 'workgroups': w[1], 'tiles' if w[0] != 2 else 'cells': w[2], 'lds_bytes': w[3]}

    def rdf(self):
        """(host read) r, g[(a, b)], n[(a, b)] of `rdf_normalise` over the frames recorded so far"""
        return rdf_normalise(self.counts(), self.type_counts, self.r_max, self.frames, self.sum_inv_volume)


# ---- time correlation functions (include/admp_hip.h admp_md_tcf; csrc/tcf_math.h, tcf_plan.h) -----------------------------------
TCF_MAX_TYPES, TCF_LAGS_PER_WORKGROUP = 8, 16
DIFFUSION_1E5_CM2_S = 1.0e4          # 1 A^2/fs = 1e-16 cm^2 / 1e-15 s = 0.1 cm^2/s = 1e4 x 1e-5 cm^2/s
LIGHT_CM_PER_FS = 2.99792458e-5      # a frequency in 1/fs divided by this is a wavenumber in 1/cm


def tcf_layout(types, tile_atoms=256):
    """per-atom types (ints; negative: not counted; at most 0..7) -> (slot_atom int32 (n_slots), tile_type int32 (n_tiles), n_types,
    atoms per type): the counted atoms sorted by type (a stable sort: inside a type in atom order), every type's run padded with
    -1 to a whole number of tiles of `tile_atoms` slots, so that every tile holds one type; a type without atoms has no tile.
    Pure numpy."""
    t = np.asarray(types)
    if t.ndim != 1 or (t.size and not np.issubdtype(t.dtype, np.integer)):
        raise ValueError('types must be a one-dimensional array of integers')
    if int(tile_atoms) != tile_atoms or tile_atoms < 64 or tile_atoms > 1024 or tile_atoms % 64:
        raise ValueError('tile_atoms must be a multiple of 64 in 64..1024')
    tile_atoms = int(tile_atoms)
    t = t.astype(np.int64)
    if t.size and t.max() >= TCF_MAX_TYPES:
        raise ValueError('at most %d types (0..%d), got type %d' % (TCF_MAX_TYPES, TCF_MAX_TYPES - 1, t.max()))
    n_types = max(int(t.max()) + 1, 1) if t.size else 1
    counts = np.bincount(t[t >= 0], minlength=n_types).astype(np.int64)
    counted = np.nonzero(t >= 0)[0]
    order = counted[np.argsort(t[counted], kind='stable')]
    slot_atom, tile_type, at = [], [], 0
    for a in range(n_types):
        n_a = int(counts[a])
        tiles = (n_a + tile_atoms - 1) // tile_atoms
        run = np.full(tiles * tile_atoms, -1, dtype=np.int32)
        run[:n_a] = order[at:at + n_a]
        at += n_a
        slot_atom.append(run)
        tile_type += [a] * tiles
    slot_atom = np.concatenate(slot_atom) if slot_atom else np.zeros(0, dtype=np.int32)
    return slot_atom.astype(np.int32), np.array(tile_type, dtype=np.int32), n_types, counts


def tcf_normalise(sums, type_counts, dt_fs):
    """sums: {'msd': (n_types, L), 'vacf': (n_types, L), 'origins': (L,)} of `CorrelationRecorder.sums`; type_counts: the atoms N_a
    of every type -> (t, msd, vacf): t = k dt_fs, msd[a] (A^2) and vacf[a] (A^2/fs^2) the sums over N_a origins[k]; a lag without
    origins and a type without atoms give zeros.  Pure numpy."""
    m, v = np.asarray(sums['msd'], dtype=np.float64), np.asarray(sums['vacf'], dtype=np.float64)
    org = np.asarray(sums['origins'], dtype=np.float64).reshape(-1)
    N = np.asarray(type_counts, dtype=np.float64).reshape(-1)
    if m.ndim != 2 or m.shape != v.shape or m.shape != (len(N), len(org)):
        raise ValueError('msd and vacf must be (%d, %d), got %s and %s' % (len(N), len(org), m.shape, v.shape))
    t = np.arange(len(org)) * float(dt_fs)
    msd, vacf = {}, {}
    for a in range(len(N)):
        norm = N[a] * org
        ok = norm > 0
        msd[a] = np.where(ok, m[a] / np.where(ok, norm, 1.0), 0.0)
        vacf[a] = np.where(ok, v[a] / np.where(ok, norm, 1.0), 0.0)
    return t, msd, vacf


def diffusion_einstein(t, msd, t_min, t_max):
    """D = slope / 6 of the least-squares line through msd(t) over t_min <= t <= t_max (A^2/fs; x DIFFUSION_1E5_CM2_S for
    1e-5 cm^2/s).  Needs two points."""
    t, msd = np.asarray(t, dtype=np.float64), np.asarray(msd, dtype=np.float64)
    sel = (t >= t_min) & (t <= t_max)
    if sel.sum() < 2:
        raise ValueError('the fit needs at least two lags in [t_min, t_max]')
    x, y = t[sel] - t[sel].mean(), msd[sel] - msd[sel].mean()
    return float((x * y).sum() / (x * x).sum()) / 6.0


def diffusion_green_kubo(t, vacf, t_max=None):
    """D = 1/3 of the trapezoid integral of vacf from 0 to t_max (None: all of t), A^2/fs -> (D, running): running[k] is the integral
    up to t[k] over 3, for judging the plateau."""
    t, vacf = np.asarray(t, dtype=np.float64), np.asarray(vacf, dtype=np.float64)
    running = np.concatenate([[0.0], np.cumsum(0.5 * (vacf[1:] + vacf[:-1]) * np.diff(t))]) / 3.0
    k = len(t) - 1 if t_max is None else int(np.nonzero(t <= t_max)[0][-1])
    return float(running[k]), running


def vdos(t, vacf, window='hann'):
    """the vibrational density of states of a velocity autocorrelation function on the lags t = k dt (fs): the cosine transform
    S_j = dt [c_0 + 2 sum_{k >= 1} w_k c_k cos(2 pi nu_j t_k)] of c = vacf / vacf[0] at nu_j = j / (2 L dt), j = 0 .. L - 1, with
    w_k = (1 + cos(pi k / L)) / 2 (window='hann': the decaying half of a Hann window) or 1 (window=None) -> (wavenumbers in 1/cm,
    S in fs)."""
    t, vacf = np.asarray(t, dtype=np.float64), np.asarray(vacf, dtype=np.float64)
    L = len(t)
    if L < 2 or vacf.shape != t.shape or vacf[0] == 0:
        raise ValueError('vdos needs at least two lags and vacf[0] != 0')
    dt = float(t[1] - t[0])
    k = np.arange(L)
    if window == 'hann':
        w = 0.5 * (1.0 + np.cos(np.pi * k / L))
    elif window is None:
        w = np.ones(L)
    else:
        raise ValueError('window must be \'hann\' or None')
    c = w * vacf / vacf[0]
    c[1:] *= 2.0
    S = dt * (np.cos(np.pi * np.outer(k, k) / L) @ c)
    return k / (2.0 * L * dt) / LIGHT_CM_PER_FS, S


class CorrelationRecorder:
    """Accumulates mean-square displacements and velocity autocorrelations per type along a run on the device, without a host read
    per frame.  `handle_owner` is any object with a handle; `types` (ints, negative: not counted, at most 8 types) and `n_lags` = L
    are fixed at construction, `dt_fs` is the time between two records (the recorder does not know the driver's step).  The object
    owns a ring (L, 2, 3, n_slots) with d and v of the last L frames in the handle's precision -- `ValueError` above
    `max_ring_bytes` -- the unwrapped displacement of every counted atom in double, its last position, one word counting large
    jumps and the accumulators (2, n_types, L) in double.  `record` is one C call (admp_md_tcf): it unwraps the frame against the
    last one (the minimum image of pos - last in the cell GIVEN, in double: wrapped and unwrapped trajectories give the same d;
    under a changing cell the displacement between two frames is the minimum image in the newer cell), stores it, and adds
    sum |d(t) - d(t - k)|^2 and sum v(t) . v(t - k) for every lag k the ring holds, in double without float atomics: a run
    repeats bit for bit.  Atoms should move less than a quarter of a cell height between two records; `info()['large_jumps']` counts
    the moves that did not.  The centre-of-mass drift is not removed."""

    def __init__(self, handle_owner, types, n_lags, dt_fs, tile_atoms=256, max_ring_bytes=2 ** 31):
        self._o = o = handle_owner
        if int(n_lags) != n_lags or n_lags < 1:
            raise ValueError('n_lags must be a positive integer')
        self.n_lags, self.dt_fs = int(n_lags), float(dt_fs)
        if not (np.isfinite(self.dt_fs) and self.dt_fs > 0):
            raise ValueError('dt_fs must be positive and finite')
        slot_atom, tile_type, self.n_types, self.type_counts = tcf_layout(types, tile_atoms)
        self.n_atoms, self.tile_atoms = len(np.asarray(types)), int(tile_atoms)
        self.n_slots, self.n_tiles = len(slot_atom), len(tile_type)
        item = torch.empty(0, dtype=o._dtype).element_size()
        self.ring_bytes = self.n_lags * 6 * self.n_slots * item
        if self.ring_bytes > max_ring_bytes:
            raise ValueError('the ring of %d lags x %d slots needs %d bytes (%.2f GiB), above max_ring_bytes = %d'
                             % (self.n_lags, self.n_slots, self.ring_bytes, self.ring_bytes / 2.0 ** 30, max_ring_bytes))
        dev = o._device
        self._slot_atom = torch.as_tensor(slot_atom).to(dev)
        self._tile_type = torch.as_tensor(tile_type).to(dev)
        # (one element at least: an empty device array has no address, and the library refuses a NULL ring or state)
        self._ring = torch.zeros(max(self.n_lags * 6 * self.n_slots, 1), dtype=o._dtype, device=dev)
        self._unwrapped = torch.zeros(max(3 * self.n_slots, 1), dtype=torch.float64, device=dev)
        self._last = torch.zeros(max(3 * self.n_slots, 1), dtype=o._dtype, device=dev)
        self._jumps = torch.zeros(1, dtype=torch.int64, device=dev)
        self._acc = torch.zeros(2 * self.n_types * self.n_lags, dtype=torch.float64, device=dev)
        self._info = (ctypes.c_int64 * 4)()
        self.frames = 0

    def record(self, positions, velocities, box):
        """one frame (positions, velocities: (n, 3) device tensors of the handle's precision; box: 9 host values, rows): one C
        call, no host read.  ValueError for what the library refuses as an argument (a singular box): nothing is recorded then."""
        o = self._o
        _checked_as(o, (self.n_atoms, 3), positions=positions, velocities=velocities)
        boxa, _ = o._harr('tcf_box', box, 9)
        o._use_current_stream()
        P = o._ptr
        rc = o._L.admp_md_tcf(o._h, self.n_atoms, P(positions), P(velocities), boxa, self.n_slots, P(self._slot_atom), self.n_tiles,
                              P(self._tile_type), self.tile_atoms, self.n_types, self.n_lags, self.frames, P(self._ring),
                              P(self._unwrapped), P(self._last), P(self._jumps), P(self._acc), self._info)
        if rc == _lib.E_ARG:
            msg = o._L.admp_last_error(o._h)
            raise ValueError('admp_md_tcf: %s' % (msg.decode() if msg else ''))
        _lib.check(o._h, rc, 'admp_md_tcf')
        self.frames += 1

    def origins(self):
        """the time origins behind every lag: max(0, frames - k)"""
        return np.maximum(0, self.frames - np.arange(self.n_lags)).astype(np.int64)

    def sums(self):
        """(host read) {'msd': (n_types, L) sums of |d(t) - d(t - k)|^2, 'vacf': (n_types, L) sums of v(t) . v(t - k), 'origins': (L,)}"""
        a = self._acc.cpu().numpy().reshape(2, self.n_types, self.n_lags)
        return {'msd': a[0].copy(), 'vacf': a[1].copy(), 'origins': self.origins()}

    def msd(self):
        """(host read) t (fs), {type: mean-square displacement in A^2}"""
        t, m, _ = tcf_normalise(self.sums(), self.type_counts, self.dt_fs)
        return t, m

    def vacf(self):
        """(host read) t (fs), {type: velocity autocorrelation in A^2/fs^2}"""
        t, _, v = tcf_normalise(self.sums(), self.type_counts, self.dt_fs)
        return t, v

    def reset(self):
        """zero accumulators and jump word (memsets on the current stream), no frames: the next record re-initialises the state"""
        self._acc.zero_()
        self._jumps.zero_()
        self.frames = 0

    def info(self):
        """what the last record launched (workgroups of the lag kernel, lags per workgroup, lags correlated, scratch bytes), the
        ring's bytes and (host read) the large jumps counted so far"""
        w = [int(x) for x in self._info]
        return {'workgroups': w[0], 'lags_per_workgroup': w[1], 'lags': w[2], 'scratch_bytes': w[3], 'ring_bytes': self.ring_bytes,
                'large_jumps': int(self._jumps.cpu().numpy().view(np.uint64)[0])}

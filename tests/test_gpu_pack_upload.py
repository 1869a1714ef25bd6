"""mphip_update_met_packed and mphip_prefetch_met_packed against mphip_update_met and mphip_prefetch_met: a snapshot whose
level fields go to the device as 16-bit codes and are decoded there steps exactly as the same snapshot uploaded as the
decoded floats -- positions, quantities and cache->uvwp agree in every bit.

Cases of tests/cases.py on the `tiny` grid (36 x 19 x 20 and the periodic column), 20 steps: `advect` (the winds only) and
`full` (turbulent and mesoscale diffusion, convection, wet and dry deposition: the cloud-water fields are consumed).  The
meteorology is first replaced by refpack.decode(refpack.encode(.)) within the reader's limits; run (a) uploads those floats,
run (b) the codes -- into a context that was created with OTHER snapshots, so that a packed upload that wrote nothing would
show.

upload_fields launches the decoder itself and carries a host code array's offset from a 16-byte boundary to the device:
the same comparison with the code arrays at every one of the eight offsets, and one snapshot pair of 257 x 241 x 70 values
(more than one pass of the decoder's grid) whose every node is read back through intpol_met."""
import copy

import numpy as np
import pytest

import cases
import refpack as R
from mptrac_amd import hip
from mptrac_amd.synth import synthetic_met
from test_gpu_pack import unaligned

pytestmark = pytest.mark.gpu
N = 2000
STEPS = 20


def limits(name):
    return hip.PACK_LIMITS.get(name, hip.PACK_LIMITS_OPEN)


def coded(met, names=None):
    """(the snapshot with the level fields `names` replaced by their decoded codes, the snapshot without them, their codes)."""
    names = tuple(met.f3) if names is None else names
    dec, bare = copy.copy(met), copy.copy(met)
    dec.f3, bare.f3, packed = dict(met.f3), dict(met.f3), {}
    for f in names:
        q, scl, off = R.encode(met.f3[f])
        dec.f3[f] = R.decode(q, scl, off, *limits(f))
        del bare.f3[f]
        packed[f] = (q, scl, off)
    return dec, bare, packed


def other(met, t):
    return synthetic_met("tiny", t, 0.37, fields=tuple(met.f3) + tuple(met.f2))


def same_state(a, b):
    sa, sb = a.state(), b.state()
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert R.same_bits(sa[k], sb[k]), k
    return sa


def run_pair(case, names_of):
    ctl, clim, m0, m1, atm = cases.make_case(case, n=N, grid="tiny")
    (d0, b0, p0), (d1, b1, p1) = (coded(m, names_of(m)) for m in (m0, m1))
    a = hip.Simulation(ctl, clim, d0, d1, atm)
    b = hip.Simulation(ctl, clim, other(m0, 0.0), other(m1, 3600.0), atm)
    try:
        b.update_met_packed(0, b0, p0)
        b.update_met_packed(1, b1, p1)
        for s in (a, b):
            s.timesteps_init(0.0, 0.0)
        times = cases.step_times(a.ctl)[:STEPS]
        assert len(times) == STEPS
        for t in times:
            a.run_timestep(t)
            b.run_timestep(t)
        state = same_state(a, b)
        assert not np.array_equal(state["lon"], atm["lon"])         # (they moved)
        return state
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("case", ["advect", "full"])
def test_codes_step_like_their_decoded_floats(case):
    state = run_pair(case, lambda m: None)
    if case == "full":
        ctl = cases.make_case(case, n=1, grid="tiny")[0]
        assert (state["q"][ctl["qnt_mloss_wet"]] > 0).any()         # (wet deposition acted: the cloud water was read)


@pytest.mark.parametrize("case", ["advect", "full"])
def test_half_of_the_fields_packed_and_half_float(case):
    run_pair(case, lambda m: tuple(sorted(m.f3))[::2])


def test_the_decoded_snapshot_is_not_the_original():
    """(the comparison above is not one of a snapshot with itself: the codes lose bits)"""
    m0 = cases.make_case("advect", n=1, grid="tiny")[2]
    dec = coded(m0)[0]
    assert not np.array_equal(dec.f3["u"], m0.f3["u"])


@pytest.mark.parametrize("case", ["advect", "full"])
def test_packed_prefetch_and_commit_equal_the_synchronous_swap(case):
    """prefetch_met_packed + commit_met against swap_met + update_met over 3 h with 4 snapshots (the shape of
    test_met_prefetch_and_commit_equal_the_synchronous_swap): the prefetch is issued right after each hand-over."""
    ctl, clim, m0, m1, atm = cases.make_case(case, n=N, grid="tiny")
    ctl["t_stop"] = 10800.0
    fields = tuple(m0.f3) + tuple(m0.f2)
    m2 = synthetic_met("tiny", 7200.0, 0.8, fields=fields)
    m3 = synthetic_met("tiny", 10800.0, 1.1, fields=fields)
    c = [coded(m) for m in (m0, m1, m2, m3)]
    a = hip.Simulation(ctl, clim, c[0][0], c[1][0], atm)
    b = hip.Simulation(ctl, clim, other(m0, 0.0), other(m1, 3600.0), atm)
    try:
        b.update_met_packed(0, c[0][1], c[0][2])
        b.update_met_packed(1, c[1][1], c[1][2])
        for s in (a, b):
            s.timesteps_init(0.0, 0.0)
        b.prefetch_met_packed(c[2][1], c[2][2])
        with pytest.raises(hip.MphipError):
            b.prefetch_met_packed(c[3][1], c[3][2])            # one snapshot at a time
        upcoming = [(3600.0, 2, 3), (7200.0, 3, None)]
        for t in cases.step_times(a.ctl):
            if upcoming and t > upcoming[0][0]:
                _, new1, after = upcoming.pop(0)
                a.swap_met(c[new1][0])
                b.commit_met()
                if after is not None:
                    b.prefetch_met_packed(c[after][1], c[after][2])
            a.run_timestep(t)
            b.run_timestep(t)
        assert not upcoming
        same_state(a, b)
    finally:
        a.close()
        b.close()


def placed(packed, shift, first="u"):
    """The codes of `packed` copied so that those of `first` start `shift` elements behind a 16-byte boundary and every
    other field's at a shift of its own (rotated): upload_fields carries each to the device in PackedField::shift."""
    out = {}
    for i, f in enumerate([first] + sorted(set(packed) - {first})):
        q, scl, off = packed[f]
        out[f] = (unaligned(q, (shift + i) % 8), scl, off)
    return out


@pytest.mark.parametrize("shift", range(8))
def test_code_arrays_at_every_alignment_step_like_their_decoded_floats(shift):
    """update_met_packed on both slots, then prefetch_met_packed + commit_met, the code arrays of u at `shift` and those of
    the other eight fields at shifts of their own; DT_MOD 900 s, 7 steps across the hand-over at 3600 s."""
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=N, grid="tiny")
    ctl.update(dt_mod=900.0, t_stop=5400.0)
    m2 = synthetic_met("tiny", 7200.0, 0.8, fields=tuple(m0.f3) + tuple(m0.f2))
    c = [coded(m) for m in (m0, m1, m2)]
    codes = [placed(p, shift) for _, _, p in c]
    assert len(codes[0]) == 9 and len({q.ctypes.data % 16 for q, _, _ in codes[0].values()}) == 8
    assert codes[0]["u"][0].ctypes.data % 16 == 2 * shift
    a = hip.Simulation(ctl, clim, c[0][0], c[1][0], atm)
    b = hip.Simulation(ctl, clim, other(m0, 0.0), other(m1, 3600.0), atm)
    try:
        b.update_met_packed(0, c[0][1], codes[0])
        b.update_met_packed(1, c[1][1], codes[1])
        for s in (a, b):
            s.timesteps_init(0.0, 0.0)
        b.prefetch_met_packed(c[2][1], codes[2])
        times = cases.step_times(a.ctl)
        assert len(times) == 7
        swapped = False
        for t in times:
            if t > 3600.0 and not swapped:
                a.swap_met(c[2][0])
                b.commit_met()
                swapped = True
            a.run_timestep(t)
            b.run_timestep(t)
            if t == 3600.0:
                same_state(a, b)
        state = same_state(a, b)
        assert swapped and not np.array_equal(state["lon"], atm["lon"])
    finally:
        a.close()
        b.close()


BIG = (256, 241, 70)        # with the periodic column 257 x 241 x 70 = 4 335 590 values: a second, ragged pass; step = 44
WINDS = ("u", "v", "w")


def test_an_upload_above_one_pass_is_seen_as_decoded_at_every_node():
    """upload_fields launches met_unpack_kernel itself; above 4 194 304 values the lanes of its first workgroups take a
    second run whose level is advanced by step = 4 194 304 mod 70 = 44.  Context A takes refpack.decode(refpack.encode(.))
    as floats, context B the codes (both snapshots of the pair); intpol_met at every node, on the snapshot's own axes and
    at each snapshot's own time, gives the same bits in both.  The node itself has weight 1 there and its neighbours 0,
    so a wrong value anywhere shows.

    Against refpack.decode itself: every blend of the interpolation is w (x - y) + y with w = 0 or 1 at a node.  w = 0
    returns y; w = 1 returns y + fl(x - y), which is x up to the rounding of the difference -- at most 2^-24 (|x| + |y|) in
    the vertical blend (a float difference) and 2^-53 (|x| + |y|) in the two horizontal ones and in time.  With M the
    largest magnitude of the field in both snapshots that is less than 2^-22 M in all; a value decoded with another
    level's scale and offset is off by a share of the level's range.  (Most nodes return the decoded float itself; the
    count of those that do not is printed: 17 990 of u, the row at the south pole where u is 1e-15 beside 0.4.)"""
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=16, grid=BIG, fields=WINDS + ("ps",))
    assert m0.f3["u"].shape == (257, 241, 70) and m0.f3["u"].size == 4335590 > 4194304 and 4194304 % 70 == 44
    (d0, b0, p0), (d1, b1, p1) = coded(m0), coded(m1)
    fields = WINDS + ("ps",)
    nx, ny, nlev = m0.f3["u"].shape
    lon, lat, p = np.repeat(m0.lon, ny * nlev), np.tile(np.repeat(m0.lat, nlev), nx), np.tile(m0.p, nx * ny)
    rows = {}
    a = hip.Simulation(ctl, clim, d0, d1, atm)
    try:
        rows["a"] = [a.intpol_met_rows(m.time, p, lon, lat, WINDS) for m in (m0, m1)]
    finally:
        a.close()
    b = hip.Simulation(ctl, clim, synthetic_met(BIG, 0.0, 0.37, fields=fields), synthetic_met(BIG, 3600.0, 0.37, fields=fields),
                       atm)
    try:
        b.update_met_packed(0, b0, p0)
        b.update_met_packed(1, b1, p1)
        rows["b"] = [b.intpol_met_rows(m.time, p, lon, lat, WINDS) for m in (m0, m1)]
    finally:
        b.close()
    for k, dec in enumerate((d0, d1)):
        assert R.same_bits(rows["a"][k], rows["b"][k]), (k, int((rows["a"][k] != rows["b"][k]).sum()))
        for j, f in enumerate(WINDS):
            ref = dec.f3[f].reshape(-1)
            got = rows["b"][k][j]
            assert np.isfinite(ref).all() and R.same_bits(dec.f3[f], R.decode(*(p0, p1)[k][f], *limits(f)))
            top = max(float(np.abs(d.f3[f]).max()) for d in (d0, d1))
            print(f, "snapshot", k, "nodes that do not return the decoded float:", int((got.astype(np.float32) != ref).sum()),
                  "largest distance / M:", float(np.abs(got - ref).max()) / top)
            assert (np.abs(got - ref) <= 2.0 ** -22 * top).all(), (f, k)
            if k == 1:          # (time weight 0 and, behind the first level, vertical weight 0)
                assert np.array_equal(got.astype(np.float32).reshape(nx, ny, nlev)[-1, -1, 1:], dec.f3[f][-1, -1, 1:])


def test_grid_dimensions_must_match_and_bad_descriptions_are_refused():
    ctl, clim, m0, m1, atm = cases.make_case("advect", n=10, grid="tiny")
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        fields = tuple(m0.f3) + tuple(m0.f2)
        small = synthetic_met((18, 10, 20), 3600.0, 1.0, fields=fields)
        _, bare, packed = coded(small)
        with pytest.raises(hip.MphipError, match="Meteo grid dimensions do not match!"):
            s.update_met_packed(1, bare, packed)
        with pytest.raises(hip.MphipError, match="Meteo grid dimensions do not match!"):
            s.prefetch_met_packed(bare, packed)
        dec, bare, packed = coded(m1)
        with pytest.raises(hip.MphipError, match="mphip_update_met_packed: field u is given both as floats and as codes"):
            s.update_met_packed(1, dec, packed)
        q, scl, off = packed["u"]
        with pytest.raises(hip.MphipError, match="mphip_update_met_packed: field u is given as codes without scl or off"):
            s.update_met_packed(1, bare, dict(packed, u=(q, None, off)))
        with pytest.raises(hip.MphipError, match="mphip_prefetch_met_packed: field u: the limits need lo <= hi"):
            s.prefetch_met_packed(bare, dict(packed, u=(q, scl, off, 2.0, 1.0)))
        # nothing was written: the context still steps as one that never saw these calls
        ref = hip.Simulation(ctl, clim, m0, m1, atm)
        try:
            for x in (s, ref):
                x.timesteps_init(0.0, 0.0)
                x.run_timestep(0.0)
                x.run_timestep(180.0)
            same_state(s, ref)
        finally:
            ref.close()
    finally:
        s.close()

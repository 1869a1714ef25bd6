"""Restatement of module_radio_depo (mphip_set_radio_depo), for the deposition tests.  This is the project's own
definition -- the reference's source was not available, as for the half-lives of tests/refradio.py.

A ground grid (lon0, lon1, nx, lat0, lat1, ny), ncell = nx * ny.  The inventory is wet[6][ncell + 1] and dry[6][ncell + 1]
in Bq, nuclides in refradio.NAMES order, cell ix * ny + iy with

    outside if lon < lon0 or lon >= lon1 or lat < lat0 or lat >= lat1
    ix = (int) ((lon - lon0) / ((lon1 - lon0) / nx)), iy likewise; outside if ix >= nx or iy >= ny

and element ncell of every row collects the deposits outside the grid.  Apb210, Abe7, Acs137 and Ai131 deposit; the noble
gases Arn222 and Axe133 never do, their rows and those of absent activities stay zero.

A step at time t:
  1. ground decay: with an earlier time t_inv, every element of nuclide k is multiplied by exp(-lambda_k (t - t_inv)) (the C
     library's exp; lambda_k of refradio.LAMBDA); then t_inv = t.  No ingrowth on the ground.
  2. for every particle with dt != 0 on which the wet or the dry deposition module acts, with the module's factor
     aux = exp(-dt lambda) as it is applied to the mass, for every depositing present activity:
         a0 = A;  wet acts: a1 = a0 * aux_w, w = a0 - a1 (else a1 = a0, w = 0)
                  dry acts: a2 = a1 * aux_d, d = a1 - a2 (else a2 = a1, d = 0);  A = a2
     every product and difference rounded once.
  3. the w and d of the particles are added per cell in ascending particle index, starting from zero; then
     inventory = inventory * f + step, as two roundings.
Nothing else changes.  The factors and which particles a module acts on are inputs: the tests take them from the oracle's
module_wet_depo / module_dry_depo on a mass of one."""
import math

import numpy as np

import refradio

NAMES = refradio.NAMES
DEPOSITING = ("Apb210", "Abe7", "Acs137", "Ai131")
NOBLE = ("Arn222", "Axe133")


def ground_cell(grid, lon, lat):
    """cell of every position (ncell = outside)"""
    lon0, lon1, nx, lat0, lat1, ny = grid
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    dlon, dlat = (lon1 - lon0) / nx, (lat1 - lat0) / ny
    out = (lon < lon0) | (lon >= lon1) | (lat < lat0) | (lat >= lat1)
    with np.errstate(invalid="ignore"):
        ix = ((np.where(out, lon0, lon) - lon0) / dlon).astype(np.int64)      # (truncation, as the C cast)
        iy = ((np.where(out, lat0, lat) - lat0) / dlat).astype(np.int64)
    out |= (ix >= nx) | (iy >= ny)
    return np.where(out, nx * ny, ix * ny + iy).astype(np.int64)


class Inventory:
    def __init__(self, grid):
        self.grid = tuple(grid)
        self.ncell = int(grid[2]) * int(grid[5])
        self.wet = np.zeros((len(NAMES), self.ncell + 1))
        self.dry = np.zeros((len(NAMES), self.ncell + 1))
        self.t_inv = None
        self.cells = None         # of the last step: cell per particle, -1 where nothing deposited
        self.step_wet = np.zeros_like(self.wet)      # of the last step: the step sums by themselves
        self.step_dry = np.zeros_like(self.dry)

    def decay_to(self, t):
        if self.t_inv is not None:
            for k in range(len(NAMES)):
                f = math.exp(-refradio.LAMBDA[k] * (t - self.t_inv))      # (math.exp is the C library's)
                self.wet[k] = self.wet[k] * f
                self.dry[k] = self.dry[k] * f
        self.t_inv = t

    def step(self, t, q, idx, lon, lat, dt, aux_w, acts_w, aux_d, acts_d):
        """One step on the quantity rows q[nq][np] in place; idx: the six row indices in NAMES order (-1: absent) or
        {name: row}.  aux_w / aux_d: the factors, acts_w / acts_d: where each module acts.  Returns self."""
        if isinstance(idx, dict):
            idx = [idx.get(n, -1) for n in NAMES]
        n = len(dt)
        f = np.ones(len(NAMES))
        if self.t_inv is not None:
            f = np.array([math.exp(-refradio.LAMBDA[k] * (t - self.t_inv)) for k in range(len(NAMES))])
        self.t_inv = t
        cell = ground_cell(self.grid, lon, lat)
        acts_w = np.asarray(acts_w, dtype=bool) & (np.asarray(dt) != 0)
        acts_d = np.asarray(acts_d, dtype=bool) & (np.asarray(dt) != 0)
        self.cells = np.where(acts_w | acts_d, cell, -1)
        self.step_wet[:], self.step_dry[:] = 0.0, 0.0
        for k, name in enumerate(NAMES):
            if name not in DEPOSITING or idx[k] < 0:
                continue
            row = q[idx[k]]
            sw, sd = np.zeros(self.ncell + 1), np.zeros(self.ncell + 1)
            for i in range(n):                                            # serial, ascending index
                if not (acts_w[i] or acts_d[i]):
                    continue
                a0 = row[i]
                a1, w, d = a0, 0.0, 0.0
                if acts_w[i]:
                    a1 = a0 * aux_w[i]
                    w = a0 - a1
                a2 = a1
                if acts_d[i]:
                    a2 = a1 * aux_d[i]
                    d = a1 - a2
                row[i] = a2
                sw[cell[i]] += w
                sd[cell[i]] += d
            self.step_wet[k], self.step_dry[k] = sw, sd
            self.wet[k] = self.wet[k] * f[k] + sw
            self.dry[k] = self.dry[k] * f[k] + sd
        return self


def serial_cell_sums(values, cell, ncell):
    """sum of values per cell in ascending index (cell < 0: left out), ncell + 1 bins"""
    out = np.zeros(ncell + 1)
    for i in np.nonzero(np.asarray(cell) >= 0)[0]:
        out[cell[i]] += values[i]
    return out

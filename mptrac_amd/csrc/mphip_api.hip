// mphip_api.hip -- C ABI of the MI355X back end (include/mptrac_hip.h):
// context, device mirrors of the reference structs, the module scheduler of
// mptrac_run_timestep and the kernel launches.  Built for gfx950 only.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "mphip_buffers.hpp"
#include "mphip_kernels.hpp"
#include "mphip_metprep.hpp"
#include "mphip_regrid.hpp"
#include "mphip_detrend.hpp"
#include "mphip_ingest.hpp"
#include "mphip_pack.hpp"
#include "mphip_intpol.hpp"

using namespace mphip;

namespace {

constexpr unsigned kAdv = MPHIP_MOD_TIMESTEPS | MPHIP_MOD_POSITION | MPHIP_MOD_ADVECT | MPHIP_MOD_POSITION2;
constexpr unsigned kAdvTurb = kAdv | MPHIP_MOD_DIFF_TURB;
constexpr unsigned kAdvDiff = kAdvTurb | MPHIP_MOD_DIFF_MESO;
constexpr unsigned kAdvTurbConvSedi = kAdvTurb | MPHIP_MOD_CONVECTION | MPHIP_MOD_SEDI;
constexpr unsigned kAdvDiffConvSedi = kAdvDiff | MPHIP_MOD_CONVECTION | MPHIP_MOD_SEDI;
// every mover behind module_advect, dt from memory (single-module sequences of a caller)
constexpr unsigned kDiffConvSediOnly = MPHIP_MOD_TIMESTEPS | MPHIP_MOD_DIFF_TURB | MPHIP_MOD_DIFF_MESO | MPHIP_MOD_CONVECTION
  | MPHIP_MOD_SEDI | MPHIP_MOD_POSITION2;
constexpr unsigned kTailOnly = MPHIP_MOD_TIMESTEPS;   // no mover: a launch of loss / decay / deposition modules only
constexpr unsigned kBound = MPHIP_MOD_BOUND_COND | MPHIP_MOD_BOUND_COND2;
constexpr unsigned kParticleBits = 0x3fffu | MPHIP_MOD_ISOSURF | kBound | MPHIP_MOD_ISOSURF_INIT;

const char *const kField3Name[MPHIP_N3D] = { "u", "v", "w", "t", "lwc", "rwc", "iwc", "swc", "pl", "ul", "vl", "zetal",
                                             "zeta_dotl", "h2o", "z", "pv", "o3", "cc", "wl" };
const char *const kField2Name[MPHIP_N2D] = { "ps", "pbl", "cape", "cin", "pel", "pct", "pcb", "cl", "ess", "nss", "shf", "ts",
                                             "zs", "us", "vs", "lsm", "sst", "pt", "tt", "zt", "h2ot", "plcl", "plfc", "o3c" };

struct MetSlot {
  bool valid = false;
  double time = 0;
  DevBuf<float> f3[MPHIP_N3D];
  DevBuf<float> f2[MPHIP_N2D];
  bool has3[MPHIP_N3D] = {};
  bool has2[MPHIP_N2D] = {};
  std::vector<double> lon, lat, p;    // the snapshot's own axes: the reference interpolates on those of the current met0
  float ps11 = 0.f;                   // ps at grid node [1][1] (module_position reflects there)
  // smallest surface pressure of the snapshot (-inf if a value is not finite: no shortcut then) and smallest
  // finite cloud-top pressure: lower bounds of what the deposition modules interpolate (DevMet::ps_skip, pct_skip)
  double ps_min = -HUGE_VAL, pct_min = -HUGE_VAL;
  // extremes of ps / pbl (all values finite, else unknown = the defaults) and the smallest pel that is not a NaN:
  // bounds of what module_diff_turb and module_convection interpolate (DevMet::turb_skip, conv_skip)
  double ps_max = HUGE_VAL, pbl_min = -HUGE_VAL, pbl_max = HUGE_VAL, pel_min = -HUGE_VAL;
};

// What mphip_derive_met, mphip_regrid_met, mphip_detrend_met, mphip_ingest_met, mphip_unpack_met and mphip_pack_met share
// (PrepCall below is one call's view of it): a stream of their own, so that a file-reader thread may call them while
// another thread steps; the lock that serialises their callers; and the scratch of the call in progress.  No buffer
// carries a value from one call to the next, so the pool hands its buffers out from the first again at every call
// (PrepCall::take); a buffer grows when a call needs more than it holds and is kept otherwise, so a repeating sequence of
// calls allocates nothing after its first round.
struct PrepState {
  std::mutex lock;
  hipStream_t stream = nullptr;
  std::vector<DevBuf<char>> pool;
  size_t taken = 0;                   // buffers of the pool the call in progress has taken
};

}   // namespace

// Every device or page-locked array below is a DevBuf / PinnedBuf (mphip_buffers.hpp): it owns its memory and its
// capacity, so `delete ctx` frees them all and no capacity is kept beside a pointer.
struct mphip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::mutex err_lock;

  mphip_ctl_t ctl;
  bool have_ctl = false;
  DevBuf<DevClim> d_clim;
  DevClim h_clim = {};               // host copy of *d_clim (DevMet::strat_skip)
  bool have_clim = false;
  DevBuf<double> d_zm[MPHIP_NZM];    // zonal-mean climatologies: [time | p | lat | vmr] each
  DevZm zm[MPHIP_NZM] = {};
  DevBuf<double> d_ts[MPHIP_NTR];    // trace-gas time series: [time | vmr] each
  DevTracerSeries h_tracers = {};    // host copy of *d_tracers
  DevBuf<DevTracerSeries> d_tracers;

  // ---- meteo ----
  MetSlot slot[2];
  int flip = 0;                       // logical slot s lives in slot[s ^ flip]
  MetSlot next;                       // snapshot being uploaded ahead of time (mphip_prefetch_met)
  bool next_pending = false;
  hipStream_t copy_stream = nullptr;  // uploads of `next` run here, beside the kernels on `stream`
  hipEvent_t next_ready = nullptr;
  hipEvent_t main_mark = nullptr;     // copies into `next` start after the kernels queued so far (they may read its arrays)
  // mphip_update_met_packed / mphip_prefetch_met_packed: where a field's {scl | off | codes} wait for met_unpack_kernel,
  // one buffer per stream ([0] stream, [1] copy_stream), sized for the largest field and reused in stream order; grow-only,
  // released with the slot arrays on a new grid
  DevBuf<char> codes[2];
  std::thread uploader;               // mphip_prefetch_met: issues the (blocking, pageable) copies beside the stepping thread
  int uploader_rc = 0;
  std::atomic<bool> uploader_done{ false };
  std::string uploader_err;
  int nx = 0, ny = 0, npl = 0, coord_type = 0;   // npl: pressure levels (met_t::np)
  int nml = 0;                                    // model levels (met_t::npl), 0 = none uploaded
  std::vector<double> h_lon, h_lat, h_p;
  DevBuf<double> d_axes;              // axes blob (layout: DevMet::axes)
  int lut_base = 0, lut_size = 0;
  size_t axes_bytes = 0;
  bool told_shortcuts_off = false;    // mphip_update_met's note about a nearly periodic longitude axis was printed
  // module_meteo only writes quantities nothing on the device reads: its launch is deferred until someone
  // can see the result (a download, gridded output, a single-module call) or its inputs change; a pending
  // launch that the next time step would overwrite unseen is dropped
  bool lazy_meteo = true;
  bool meteo_pending = false;

  // ---- packed grids ----
  // Packed two-snapshot grids (layouts: mphip_device.hpp).  `pk` is the set the kernels read; `pk_next` is
  // built beside the time steps from (met1, prefetched snapshot) on the copy stream and trades places with it
  // in mphip_commit_met, so that a hand-over costs the stepping stream nothing.
  struct PackedGrids {
    DevBuf<float> wind, temp, h2o;
    DevBuf<float> mlw, zl2, pl2;      // model levels: {ul,vl,zeta_dot|wl}, {zetal}, {pl} pairs
    DevBuf<f32x4> mx, mx2;            // level / surface pair records of module_meteo
    DevBuf<f32x4> cloud, sfa, sfb, sfc, sfd;
    DevBuf<f32x4> cp2;                // {cape,pel} pair records (module_convection)
    DevBuf<int> ml_mono;              // cleared by the pack kernel if a height column is not monotonic
    bool ml_monotonic = false;
    // module_diff_meso's wind deviations per raw cell (DevMet::meso), a function of `wind` alone: valid for exactly the
    // records it was built from (pack_launch, which writes `wind`, voids or rebuilds it; ensure_meso_table builds it for a
    // set packed while the module was off).  Allocated only in a context whose control parameters switch the module on.
    DevBuf<float> meso;
    bool meso_valid = false;
  };
  PackedGrids pk, pk_next;
  bool pk_next_valid = false;         // pk_next holds (met1, prefetched snapshot), packed with the control parameters of then
  bool packed_dirty = true;

  // ---- particles ----
  long long np = 0, ip0 = 0, np_total = 0;
  int nq = 0;
  DevBuf<double> d_arr[4 + MPHIP_NQ_MAX];   // time, p, lon, lat, q[*]
  DevBuf<double> d_alt[4 + MPHIP_NQ_MAX];   // gather targets (ping-pong)
  DevBuf<float> d_uvwp[3], d_uvwp_alt[3];
  DevBuf<double> d_dt, d_dt_alt;
  uint64_t rng_ctr = 0;
  DevBuf<double> d_iso, d_iso_alt;          // cache->iso_var (allocated on first use)
  DevBuf<int> d_kz, d_kz_alt;               // model-level search hint per particle (allocated on first use)
  DevBuf<double> d_iso_ts, d_iso_ps;        // balloon time series (ISOSURF 4)
  int iso_n = 0;
  // One page-locked span of caller memory (option pin_host_atm: the particle arrays of a persistent atm_t,
  // which lie next to each other in one allocation); released by mphip_destroy.
  std::vector<std::pair<uintptr_t, uintptr_t>> pinned;
  std::mutex pinned_lock;

  // ---- locality order ----
  // internal locality order: particles are stored sorted by meteo grid cell;
  // d_ext[i] is the external slot (the reference's ip) of stored particle i
  DevBuf<int> d_ext, d_ext_alt;
  bool ext_identity = true;
  int steps_since_resort = 1 << 30;
  const int *fold_perm = nullptr;     // the locality re-sort's permutation, handed to the multi-step launch that follows
                                      // it inside one mphip_run_timesteps iteration (DevAtm::perm_all)
  DevBuf<f32x4u> d_prec;              // permute_random: one record per particle (option perm_records)

  // ---- sort / repair / sort ahead ----
  DevBuf<uint32_t> d_keys[2];
  DevBuf<int> d_vals[2];
  DevBuf<uint32_t> d_counts;
  int sorted_buf = -1;                // which d_keys/d_vals pair holds the last result
  const int *fused_perm = nullptr;    // set by do_sort, consumed by the next launch_step
  // the counters of the step kernel's chunk queues (kQueueInts; zero between launches: the kernel's last wave zeroes
  // them) and the workgroups of an instantiation that a CU holds at a time, by kernel and dynamic LDS size
  DevBuf<int> d_step_queue;
  std::map<std::pair<const void *, size_t>, int> step_resident;
  bool fused_quantities = false;      // ... which then moves the quantity arrays too (option fuse_sort_quantities)
  // module_sort as a repair of the previous order (repair_* kernels): valid while the particles are stored in the order
  // of the last module_sort (stored_is_sorted) -- its sorted keys are then non-decreasing along the slots
  bool stored_is_sorted = false;
  long long sorted_n = 0;
  DevBuf<uint32_t> rep_sk, rep_mk[2], rep_fk, rep_tiles, rep_nm;
  DevBuf<int> rep_si, rep_mi[2], rep_fv;
  // module_sort of the NEXT time step, started beside the rest of this one (option "sort_ahead"): once the launch
  // that moves the particles has run, their positions are final for this step -- module_mixing and the deposition
  // modules only change quantities -- so the keys and the radix sort of the next step's module_sort (and its
  // module_timesteps) can run on a second stream, into buffers of their own, while the main stream does the
  // rest of the step.  The next mphip_run_timestep takes the result if it is called with the expected time and
  // nothing touched the particles, the grids or the control parameters in between; otherwise it is dropped.
  // The buffers trade places with d_keys / d_vals / d_counts / d_dt around the sort (ahead_swap_buffers).
  hipStream_t ahead_stream = nullptr;
  hipEvent_t ahead_mark = nullptr, ahead_done = nullptr;
  DevBuf<uint32_t> ahead_keys[2];
  DevBuf<int> ahead_vals[2];
  DevBuf<uint32_t> ahead_counts;
  DevBuf<double> ahead_dt;
  bool ahead_valid = false;
  double ahead_t = 0;
  int ahead_cur = 0;
  bool ahead_repaired = false;                     // the sort ahead repaired the previous order (it did not sort from scratch)
  long long sorts_repaired = 0, sorts_scratch = 0; // module_sort calls answered by the repair / sorted from scratch (mphip_get_sort_counts)
  long long sorts_undone = 0;                      // ... of the latter, those that found the internal locality order and undid it first
  DevBuf<unsigned char> d_depo_busy;               // EmitKeys::depo_busy (np bytes) ...
  bool depo_busy_valid = false;                    // ... written by the last launch, not yet used by its step's deposition launch
  const unsigned char *depo_busy_last = nullptr;   // ... as the step's deposition launch has just used it
  unsigned depo_busy_last_mask = 0;                // ... and the deposition modules it was decided for

  // ---- mixing and sums ----
  DevBuf<int> d_cell;
  DevBuf<double> d_sums;
  DevBuf<int> d_cnt;                  // particles per mixing cell (32-bit: the reference's `int count[]`)
  DevBuf<unsigned long long> d_lists; // work space of the ordered sums (sequence, runs, sort buffers)
  DevBuf<double> d_rec;               // mphip_grid_sums: the quantities as one record per particle (GridVals::rec)
  PinnedBuf<double> h_sums;           // page-locked staging of mphip_grid_sums and of the analysis outputs
  DevBuf<double> d_grid_kernel;       // GRID_KERNEL: kz[nk] | kw[nk] (mphip_set_grid_kernel)
  int grid_nk = 0;

  // ---- chemistry ----
  // module_chem_grid: [press nz | area ny | lon nx | lat ny] of the chemistry grid, built by mphip_update_ctl with the
  // C library's exp and cos when the grid is due and valid (chemgrid_ok)
  DevBuf<double> d_chemgrid;
  bool chemgrid_ok = false;
  double h2o2_low = 0;                // module_h2o2_chem: pow(1 / a, 1 / b) of the host's C library
  // module_tracer_chem: the photolysis rates, [p | sza | o3c | (pad) | PhotoRec rec[np][nsza][no3c]]
  // (mphip_update_clim_photo); photo_have[k]: the table of trace gas k (MPHIP_TR_CCL4 ... MPHIP_TR_N2O) was given
  DevBuf<double> d_photo;
  DevPhoto photo = {};
  bool photo_have[4] = {};

  // ---- radio ----
  // module_radio_decay (mphip_set_radio_decay): the activities (-1: absent; module_mixing mixes the present ones) and the
  // switch of the time step
  RadioQnt radio = { { -1, -1, -1, -1, -1, -1 } };
  bool radio_on = false;
  // module_radio_depo (mphip_set_radio_depo): the switch of the time step, the ground grid, this rank's part of the
  // inventory [2][MPHIP_NRADIO][rdepo_ntot] (rdepo_ntot = nx ny + 1: the last element of a plane is the bin outside the
  // grid) and the time it is valid for (rdepo_have_t: one is known)
  bool rdepo_on = false;
  mphip_box_t rdepo_grid = {};
  DevBuf<double> d_rdepo_inv;
  size_t rdepo_ntot = 0;
  bool rdepo_have_t = false;
  double rdepo_t = 0;

  // ---- analysis outputs (mphip_box_sums, mphip_sample_obs, mphip_station_hits) ----
  DevBuf<double> d_ana_kernel;        // the call's weighting function: kz[nk] | kw[nk]
  DevBuf<uint32_t> d_marks;           // counts per external index (np + 1), then their scan; chunk offsets behind them
  DevBuf<int> d_slot_of;              // station: where the particle of an external index is stored
  DevBuf<uint32_t> d_ana_flags;       // [bad member | records (scan) | records (64-bit sum, 2 words)]
  // mphip_select_atm: [slot | external index] of the selected particles by rank, the two rows in flight on the device and
  // their page-locked landing places, the events behind the copies into those
  DevBuf<int> d_sel_list;
  DevBuf<double> d_sel_rows;
  PinnedBuf<double> h_sel_rows;
  hipEvent_t sel_copied[2] = { nullptr, nullptr };

  // ---- exchange ----
  mphip_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  void *comm = nullptr;               // RCCL communicator (ncclComm_t) of mphip_comm_init, NULL = single rank / hook
  int comm_ranks = 1, comm_rank = 0;
  // exchange of the occupied levels only (exchange_occupied_levels): per-level occupancy on the device and for the host,
  // the dense band of the sums and of the counts, what was found
  DevBuf<double> d_occ, d_band;
  PinnedBuf<double> h_occ;
  DevBuf<int> d_band_cnt;
  int mix_band_lo = -1, mix_band_hi = -1;

  // mphip_derive_met, mphip_regrid_met, mphip_detrend_met: their stream, lock and scratch
  PrepState prep;

  // mphip_intpol_met: the points {time | p | lon | lat} and the values [nfield] of one chunk (grow-only)
  DevBuf<double> d_ip_in, d_ip_out;

  // ---- options (mphip_set_option; documented in include/mptrac_hip.h) ----
  int locality_interval = 60;         // re-sort every this many steps (0 = keep the caller's order)
  bool locality_zorder = false;       // tiles of the locality key numbered along a Z-order curve instead of row by row
  int locality_tile = 0;              // horizontal tile edge of the locality key (columns); 0 = 4, or 8 with model-level winds
  int step_blocks = 8192;             // upper bound of the step kernel's grid
  int step_blocks_multi = 32768;      // ... of a multi-step launch (mphip_run_timesteps)
  bool xcd_map = true;
  // the step kernel's waves claim 64-particle chunks from queues (step_queue_grid): 1 = where a launch has 16 chunks
  // or more per wave of the resident grid, 2 = in every launch (tests), 0 = never (the static partition of block_geom)
  int step_queue = 1;
  bool big_grid = false;              // take the 64-bit-offset (kBigGrid) instantiations on a grid that fits 32 bits too (tests)
  bool force_generic = false;         // "generic_kernel"
  int multi_step = 64;                // mphip_run_timesteps: most time steps per launch (0 = always one by one)
  bool fold_resort = true;            // ... and a launch that follows the locality re-sort does its gather (0: a pass of its own)
  int lds_tile = 0;                   // cells of the LDS wind tile of traj_tile_kernel (0: off); runs of pure trajectory steps only
  bool turb_strat = true;             // module_diff_turb's short path above every tropopause (DevMet::strat_skip; 0: never taken)
  bool compact_depo = true;           // deposition-only launches through depo_kernel (0: the fused kernel's tail)
  bool pin_host_atm = false;          // page-lock the caller's particle arrays (persistent atm_t of a C caller only)
  bool perm_records = true;           // random permutations of the particle arrays through records (permute_random)
  bool fuse_sort = true;              // module_sort's gather of time, p, lon, lat inside the following step launch
  bool fuse_quantities = true;        // "fuse_sort_quantities": ... which then moves the quantity arrays too
  int sort_bits = 0;                  // digit width of the radix sort (0 = fewest passes; 8, 9, 10: tuning / tests)
  bool sort_repair = true;
  bool sort_ahead = true;
  bool ahead_box = true;              // the key kernel of the sort ahead also writes module_mixing's box index (0: own kernel; 2.26 vs 2.29 ms on C5)
  bool ahead_priority = false;        // the stream of the sort ahead at the highest priority (C5: no difference, profiles/r05_variants.txt item 3)
  bool emit_keys = true;              // the launch that moves the particles writes the keys of the sort ahead
  int deterministic_sums = 1;         // cell sums in the reference's serial order (0: floating-point atomics)
  int sum_path = 0;                   // ordered sums: 0 = by crowding, 1 = groups of cells per wave, 2 = a lane per (cell, value)
  bool grid_records = true;
  int chain_blocks = 0;               // workgroups of the chain walk of the ordered sums (0: default; tuning)
  // (default 0): measured with a one-rank communicator, the band costs 0.14 ms per step (the host reads the occupancy:
  // the one synchronisation in the step path; pack / unpack) against a MODELLED saving of 0.15-0.2 ms on eight GPUs --
  // undecidable without xGMI, so the whole-grid all-reduce stays the default
  bool mix_exchange_levels = false;
  int derive_profile_phase = 0;       // what mphip_profile_begin / _end time of a preprocessing call
  int intpol_chunk = 1 << 22;         // points per launch of mphip_intpol_met: device memory does not grow with n
  bool select_direct = false;         // mphip_select_atm copies into the caller's arrays (0: through the page-locked rows)
  int select_profile_phase = 0;       // what mphip_profile_begin / _end time of mphip_select_atm

  // ---- profiling of the fused step kernel ----
  bool prof = false;
  std::vector<hipEvent_t> ev;         // start/stop pairs
  size_t ev_used = 0;
};

namespace {

int fail(mphip_ctx *ctx, const std::string &msg) {
  if (ctx) {   // (the uploader thread of mphip_prefetch_met reports through here too)
    std::lock_guard<std::mutex> guard(ctx->err_lock);
    ctx->err = msg;
  }
  return 1;
}

#define HIPCHK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(ctx, std::string(#call) + ": " + hipGetErrorString(e_));                   \
  } while (0)

// One start/stop pair of what mphip_profile_begin / _end time: the start event is recorded on `stream` here, *stop is for
// the caller to record behind what the pair brackets (NULL: nothing is being profiled).  ctx->ev grows as needed.
int prof_pair(mphip_ctx *ctx, hipStream_t stream, hipEvent_t *stop) {
  *stop = nullptr;
  if (!ctx->prof)
    return 0;
  while (ctx->ev_used + 2 > ctx->ev.size()) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    ctx->ev.push_back(e);
  }
  HIPCHK(hipEventRecord(ctx->ev[ctx->ev_used++], stream));
  *stop = ctx->ev[ctx->ev_used++];
  return 0;
}

// the raw pointers of a pair of buffers, as radix_passes takes them
template <typename T>
struct RawPair {
  T *q[2];
  explicit RawPair(DevBuf<T> (&b)[2]) : q{ b[0].p, b[1].p } {}
};

int grid_for(long long n, int block = 256, int maxb = 8192) {
  long long b = (n + block - 1) / block;
  if (b < 1)
    b = 1;
  if (b > maxb)
    b = maxb;
  return (int) b;
}

DevAtm dev_atm(const mphip_ctx *c) {
  DevAtm a;
  a.time = c->d_arr[0].p;
  a.p = c->d_arr[1].p;
  a.lon = c->d_arr[2].p;
  a.lat = c->d_arr[3].p;
  for (int iq = 0; iq < MPHIP_NQ_MAX; iq++)
    a.q[iq] = iq < c->nq ? c->d_arr[4 + iq].p : nullptr;
  a.up = c->d_uvwp[0].p;
  a.vp = c->d_uvwp[1].p;
  a.wp = c->d_uvwp[2].p;
  a.dt = c->d_dt.p;
  a.ext = c->ext_identity ? nullptr : c->d_ext.p;
  a.iso = c->d_iso.p;
  a.kz = c->d_kz.p;
  a.iso_ts = c->d_iso_ts.p;
  a.iso_ps = c->d_iso_ps.p;
  a.iso_n = c->iso_n;
  a.perm = c->fold_perm ? c->fold_perm : c->fused_perm;
  a.s_time = c->d_alt[0].p;
  a.s_p = c->d_alt[1].p;
  a.s_lon = c->d_alt[2].p;
  a.s_lat = c->d_alt[3].p;
  a.nq_perm = c->fold_perm || (c->fused_perm && c->fused_quantities) ? c->nq : 0;
  a.perm_all = c->fold_perm ? 1 : 0;   // (locality_sort_apply: the pre-sort arrays are the alternates)
  a.s_up = c->d_uvwp_alt[0].p;
  a.s_vp = c->d_uvwp_alt[1].p;
  a.s_wp = c->d_uvwp_alt[2].p;
  a.s_dt = c->d_dt_alt.p;
  a.s_ext = c->d_ext_alt.p;
  a.ext_out = c->d_ext.p;
  for (int iq = 0; iq < MPHIP_NQ_MAX; iq++)
    a.s_q[iq] = iq < c->nq ? c->d_alt[4 + iq].p : nullptr;
  a.np = c->np;
  a.ip0 = c->ip0;
  a.np_total = c->np_total;
  return a;
}

// Can the reference's horizontal weights leave [0, 1] on this grid?  Not on a Cartesian grid (both coordinates are
// clamped), and not on a longitude axis that spans the circle and starts in [-360, 0]: one shift by 360 degrees
// (intpol_check_lon_lat) then always lands inside.  A span below 360 by any amount leaves a gap.
static bool weights_stay_inside(int coord_type, double first, double last) {
  return coord_type != 0 || (last - first >= 360.0 && first <= 0.0 && first >= -360.0);
}

// The smallest tropopause pressure clim_tropo_at can return at a latitude in [-90, 90] and a second of the year in
// [0, 365.25 d].  Inside a latitude interval the value lies between the interval's nodes; in time it is A + s (B - A),
// linear in s, with s in [0, 1] inside the month axis and beyond that before the first and behind the last node (the
// first and the last interval are continued to the ends of the year).  So the minimum is at a latitude node and at an
// end of s of some month interval.  +inf (no bound) for a table the argument does not cover.
static double clim_tropo_min(const DevClim &h) {
  const double year = 365.25 * 86400.;
  if (h.ntime < 2 || h.nlat < 2 || !(h.lat[0] <= -90.0 && h.lat[h.nlat - 1] >= 90.0))
    return HUGE_VAL;
  for (int i = 0; i + 1 < h.ntime; i++)
    if (!(h.time[i] < h.time[i + 1]))
      return HUGE_VAL;
  for (int j = 0; j + 1 < h.nlat; j++)
    if (!(h.lat[j] < h.lat[j + 1]))
      return HUGE_VAL;
  double lo = HUGE_VAL;
  for (int i = 0; i + 1 < h.ntime; i++) {
    const double w = h.time[i + 1] - h.time[i];
    const double s0 = i == 0 ? std::min(0.0, (0.0 - h.time[0]) / w) : 0.0;
    const double s1 = i + 2 == h.ntime ? std::max(1.0, (year - h.time[i]) / w) : 1.0;
    for (int j = 0; j < h.nlat; j++) {
      const double a = h.tropo[i][j], b = h.tropo[i + 1][j];
      for (double s : { s0, s1 }) {
        const double v = a + s * (b - a);
        if (!(v == v))
          return HUGE_VAL;
        lo = std::min(lo, v);
      }
    }
  }
  return lo;
}

DevMet dev_met(const mphip_ctx *c) {
  DevMet M;
  M.wind = c->pk.wind.p;
  M.temp = c->pk.temp.p;
  M.cloud = c->pk.cloud.p;
  M.mx = c->pk.mx.p;
  M.mx2 = c->pk.mx2.p;
  M.sfa = c->pk.sfa.p;
  M.sfb = c->pk.sfb.p;
  M.cp2 = c->pk.cp2.p;
  M.sfc = c->pk.sfc.p;
  M.sfd = c->pk.sfd.p;
  M.h2o = c->pk.h2o.p;
  M.mlw = c->pk.mlw.p;
  M.zl2 = c->pk.zl2.p;
  M.pl2 = c->pk.pl2.p;
  M.meso = c->pk.meso_valid ? c->pk.meso.p : nullptr;
  M.meso_nty = (c->ny + 2) / 4;   // (ny - 1 cells in bricks of four, rounded up)
  M.ml_monotonic = c->pk.ml_monotonic ? 1 : 0;
  for (int t = 0; t < 2; t++) {
    M.zl[t] = c->slot[t ^ c->flip].f3[MPHIP_ZETAL].p;
    M.pll[t] = c->slot[t ^ c->flip].f3[MPHIP_PL].p;
  }
  M.npl = c->nml;
  M.axes = c->d_axes.p;
  M.lut_base = c->lut_base;
  M.lut_size = c->lut_size;
  M.lat_x0 = c->h_lat[0];
  M.lat_inv_dx = (c->ny - 1) / (c->h_lat[c->ny - 1] - c->h_lat[0]);
  M.nx = c->nx;
  M.ny = c->ny;
  M.np = c->npl;
  M.coord_type = c->coord_type;
  M.time0 = c->slot[0 ^ c->flip].time;
  M.time1 = c->slot[1 ^ c->flip].time;
  M.inv_dtime = 1.0 / (M.time1 - M.time0);
  double latmin = c->h_lat[0], latmax = c->h_lat[0];
  for (double v : c->h_lat) {
    latmin = std::min(latmin, v);
    latmax = std::max(latmax, v);
  }
  M.latmin = latmin;
  M.latmax = latmax;
  M.local = (std::fabs(c->h_lon[c->nx - 1] - c->h_lon[0] - 360.0) >= 0.01);
  // direction test of locate_irr at its first midpoint (mptrac.c:3502-3504)
  const int my = (c->ny - 1) >> 1, mp = (c->npl - 1) >> 1;
  M.lat_ascending = c->h_lat[my] < c->h_lat[my + 1];
  M.p_ascending = c->h_p[mp] < c->h_p[mp + 1];
  M.lon_first = c->h_lon[0];
  M.lon_last = c->h_lon[c->nx - 1];
  M.inv_dlon0 = 1.0 / (c->h_lon[1] - c->h_lon[0]);
  M.lat_search_max = std::nextafter(latmax, -HUGE_VAL);
  M.p_min = *std::min_element(c->h_p.begin(), c->h_p.end());
  M.p_search_max = std::nextafter(*std::max_element(c->h_p.begin(), c->h_p.end()), -HUGE_VAL);
  M.p_cmp_off = M.p_ascending ? 1 : 0;
  M.p_step = M.p_ascending ? 1 : -1;
  M.ps11[0] = c->slot[0 ^ c->flip].ps11;
  M.ps11[1] = c->slot[1 ^ c->flip].ps11;
  // a little below the smallest value of either snapshot: what lies below that is below every interpolated value
  M.ps_skip = std::min(c->slot[0].ps_min, c->slot[1].ps_min) - 1e-6;
  M.pct_skip = std::min(c->slot[0].pct_min, c->slot[1].pct_min) - 1e-6;
  // module_diff_turb / module_convection: bounds below which the boundary layer / the convective column cannot
  // reach, from the extremes of ps and pbl over both snapshots (p1 = pbl - trans (ps - pbl) is linear in both:
  // its smallest value is at a corner of the box of extremes) and the smallest pel
  {
    const double ps_lo = std::min(c->slot[0].ps_min, c->slot[1].ps_min), ps_hi = std::max(c->slot[0].ps_max, c->slot[1].ps_max);
    const double pbl_lo = std::min(c->slot[0].pbl_min, c->slot[1].pbl_min),
                 pbl_hi = std::max(c->slot[0].pbl_max, c->slot[1].pbl_max);
    auto p1_min = [&](double trans) {
      double lo = HUGE_VAL;
      for (double pbl : { pbl_lo, pbl_hi })
        for (double ps : { ps_lo, ps_hi })
          lo = std::min(lo, pbl - trans * (ps - pbl));
      return lo;
    };
    const bool known = std::isfinite(ps_lo) && std::isfinite(ps_hi) && std::isfinite(pbl_lo) && std::isfinite(pbl_hi);
    M.turb_skip = -HUGE_VAL;
    M.conv_skip = -HUGE_VAL;
    if (known && c->have_ctl) {
      const double b = std::min({ ps_lo, pbl_lo, p1_min(c->ctl.turb_pbl_trans) });
      M.turb_skip = b - 1e-6 * std::fabs(b) - 1e-6;
      double lo = ps_lo;
      if (c->ctl.conv_mix_pbl)
        lo = std::min(lo, p1_min(c->ctl.conv_pbl_trans));
      if (c->ctl.conv_cape >= 0)
        lo = std::min(lo, std::min(c->slot[0].pel_min, c->slot[1].pel_min));
      if (lo == lo)
        M.conv_skip = lo - 1e-6 * std::fabs(lo) - 1e-6;
    }
  }
  // All four bounds rest on "an interpolated value is not below the smallest node value", which needs horizontal
  // weights inside [0, 1].  The latitude is always clamped and so is the longitude of a Cartesian grid, but
  // intpol_check_lon_lat only shifts a longitude by 360 degrees: on an axis that does not span the circle (a regional
  // grid, or a first longitude above 0 or below -360) the shifted value can lie outside the axis, locate_reg clamps
  // the index, and the interpolation continues the end cell's slope -- below every node value.  A particle that left
  // such a domain within the step still has its dt.  No shortcut there (tests/depo_cases.py: extrap-regional-*).
  if (!weights_stay_inside(c->coord_type, c->h_lon[0], c->h_lon[c->nx - 1]))
    M.ps_skip = M.pct_skip = M.turb_skip = M.conv_skip = -HUGE_VAL;
  // module_diff_turb's short path (diff_turb_fast): below this pressure, at a latitude in [-90, 90], a particle is
  // above 0.866877899 x every tropopause pressure of the climatology -- tropo_weight_pt's upper edge.  It needs what
  // the boundary-layer bound needs, parameters with which "weight 1 of the stratosphere" means its parameters exactly
  // (finite, not negative; a finite transition factor of pbl_weight), no horizontal diffusion there (the path takes no
  // horizontal step), the tropopause looked up at the particle's latitude, and an axis top (where the probes of the Kz
  // gradient are clamped to) inside both regimes.
  M.strat_skip = -HUGE_VAL;
  if (c->turb_strat && c->have_ctl && c->have_clim && M.turb_skip > -HUGE_VAL && c->ctl.met_coord_type == 0) {
    const mphip_ctl_t &k = c->ctl;
    bool ok = std::isfinite(k.turb_pbl_trans);
    for (double v : { k.turb_dx_pbl, k.turb_dx_trop, k.turb_dx_strat, k.turb_dz_pbl, k.turb_dz_trop, k.turb_dz_strat })
      ok = ok && std::isfinite(v) && v >= 0;
    ok = ok && k.turb_dx_strat == 0;
    const double b = 0.866877899 * clim_tropo_min(c->h_clim);
    const double bound = b - 1e-6 * std::fabs(b) - 1e-6;
    const double ptop = c->h_p[c->npl - 1] * 1.01;
    if (ok && std::isfinite(bound) && ptop < bound && ptop < M.turb_skip)
      M.strat_skip = bound;
  }
  M.meso_dt = std::fabs(c->ctl.dt_mod);
  M.meso_r = 1 - 2 * M.meso_dt / c->ctl.dt_met;
  M.meso_r2 = std::sqrt(1 - M.meso_r * M.meso_r);
  if (!c->have_ctl || !(M.meso_dt > 0) || !std::isfinite(M.meso_r2))
    M.meso_dt = -1;    // never equal to |dt|: the kernels compute the coefficients themselves
  return M;
}

size_t axes_lds_bytes(const mphip_ctx *c) {
  return c->axes_bytes;
}

// the reference's bisection (mptrac.c:3495-3521), host copy for the look-up table
int host_locate_irr(const std::vector<double> &xx, double x) {
  const int n = (int) xx.size();
  int lo = 0, hi = n - 1;
  int mid = (hi + lo) >> 1;
  if (xx[mid] < xx[mid + 1]) {
    while (hi > lo + 1) {
      mid = (hi + lo) >> 1;
      if (xx[mid] > x)
        hi = mid;
      else
        lo = mid;
    }
  } else {
    while (hi > lo + 1) {
      mid = (hi + lo) >> 1;
      if (xx[mid] <= x)
        hi = mid;
      else
        lo = mid;
    }
  }
  return lo;
}

// axes, reciprocal interval widths and the pressure look-up table in one blob
int upload_axes(mphip_ctx *ctx) {
  const int nx = ctx->nx, ny = ctx->ny, np = ctx->npl;
  const size_t nd = 2 * (size_t) (nx + ny + np);
  std::vector<int16_t> lut;
  ctx->lut_base = ctx->lut_size = 0;
  const double pmin = *std::min_element(ctx->h_p.begin(), ctx->h_p.end());
  const double pmax = *std::max_element(ctx->h_p.begin(), ctx->h_p.end());
  if (pmin > 0 && std::isfinite(pmax) && np < 32000) {
    long long kmin, kmax;
    memcpy(&kmin, &pmin, 8);
    memcpy(&kmax, &pmax, 8);
    kmin >>= 45;
    kmax >>= 45;
    if (kmax - kmin + 1 <= 8192) {
      ctx->lut_base = (int) kmin;
      ctx->lut_size = (int) (kmax - kmin + 1);
      lut.resize((size_t) ctx->lut_size);
      for (int j = 0; j < ctx->lut_size; j++) {
        const long long bits = (kmin + j) << 45;
        double edge;
        memcpy(&edge, &bits, 8);
        lut[(size_t) j] = (int16_t) host_locate_irr(ctx->h_p, edge);
      }
    }
  }
  const size_t bytes = ((nd * sizeof(double) + lut.size() * sizeof(int16_t)) + 15) & ~(size_t) 15;
  std::vector<double> blob(bytes / sizeof(double), 0.0);
  double *b = blob.data();
  std::copy(ctx->h_lon.begin(), ctx->h_lon.end(), b);
  std::copy(ctx->h_lat.begin(), ctx->h_lat.end(), b + nx);
  std::copy(ctx->h_p.begin(), ctx->h_p.end(), b + nx + ny);
  double *inv = b + nx + ny + np;
  for (int i = 0; i + 1 < nx; i++)
    inv[i] = 1.0 / (ctx->h_lon[i + 1] - ctx->h_lon[i]);
  for (int i = 0; i + 1 < ny; i++)
    inv[nx + i] = 1.0 / (ctx->h_lat[i + 1] - ctx->h_lat[i]);
  for (int i = 0; i + 1 < np; i++)
    inv[nx + ny + i] = 1.0 / (ctx->h_p[i + 1] - ctx->h_p[i]);
  if (!lut.empty())
    memcpy(b + nd, lut.data(), lut.size() * sizeof(int16_t));
  HIPCHK(ctx->d_axes.resize(blob.size()));
  HIPCHK(hipMemcpyAsync(ctx->d_axes.p, blob.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->axes_bytes = bytes;
  return 0;
}

// arrays of a packed set for the fields the two snapshots carry (allocated on first need; an allocation, so
// called from the stepping thread only)
struct PackPlan {
  bool cloud = false, ml = false, pbl = false, mx = false, mx2 = false, ml_heights = false, coord2 = false;
  bool meso = false;   // build the table of module_diff_meso's wind deviations behind the wind records
};

// The table of module_diff_meso's wind deviations (DevMet::meso): three floats per cell, in bricks of 4 x 4 columns
static size_t meso_table_floats(const mphip_ctx *ctx) {
  return (size_t) ((ctx->nx + 2) / 4) * (size_t) ((ctx->ny + 2) / 4) * (size_t) (ctx->npl - 1) * 16 * 3;
}
static bool lean32_ok(const mphip_ctx *ctx);
// ... is built with the packed set where the control parameters switch the module on and the lean instantiations
// with 32-bit offsets, its readers, can run on the grid
static bool meso_table_wanted(const mphip_ctx *ctx) {
  // (the condition of the time step's module set, plan_step; a caller that runs the module on its own with
  // `diffusion` off gets the table in front of its first launch)
  return ctx->have_ctl && ctx->ctl.diffusion && (ctx->ctl.turb_mesox > 0 || ctx->ctl.turb_mesoz > 0)
    && lean32_ok(ctx);
}

PackPlan pack_plan(const mphip_ctx *ctx, const MetSlot &s0, const MetSlot &s1) {
  PackPlan P;
  const MetSlot *ss[2] = { &s0, &s1 };
  for (int t = 0; t < 2; t++) {
    for (int f = MPHIP_LWC; f <= MPHIP_SWC; f++)
      P.cloud = P.cloud || ss[t]->has3[f];
    for (int f = MPHIP_Z; f <= MPHIP_CC; f++)
      P.mx = P.mx || ss[t]->has3[f];
    for (int f = MPHIP_TS; f <= MPHIP_O3C; f++)
      P.mx2 = P.mx2 || ss[t]->has2[f];
    P.ml = P.ml || ss[t]->has3[MPHIP_UL] || ss[t]->has3[MPHIP_VL] || ss[t]->has3[MPHIP_ZETA_DOTL] || ss[t]->has3[MPHIP_WL];
    P.pbl = P.pbl || ss[t]->has3[MPHIP_H2O] || ss[t]->has2[MPHIP_ESS] || ss[t]->has2[MPHIP_NSS] || ss[t]->has2[MPHIP_SHF];
  }
  P.ml = P.ml && (size_t) ctx->nx * ctx->ny * ctx->nml > 0;
  // packed height pairs: {zetal}, {pl}; ADVECT_VERT_COORD 2 searches in pl only
  P.coord2 = ctx->have_ctl && ctx->ctl.advect_vert_coord == 2;
  P.ml_heights = P.ml && s0.has3[MPHIP_PL] && s1.has3[MPHIP_PL]
    && (P.coord2 || (s0.has3[MPHIP_ZETAL] && s1.has3[MPHIP_ZETAL]));
  P.meso = meso_table_wanted(ctx);
  return P;
}

int pack_alloc(mphip_ctx *ctx, mphip_ctx::PackedGrids &K, const PackPlan &P) {
  const size_t ncell = (size_t) ctx->nx * ctx->ny * ctx->npl, ncol = (size_t) ctx->nx * ctx->ny;
  const size_t ncell_ml = (size_t) ctx->nx * ctx->ny * ctx->nml;
  // (a set is released on a new grid, so every size below is the only one its array ever has: reserve = first need)
  if (P.ml) {
    HIPCHK(K.mlw.reserve(6 * ncell_ml));
    HIPCHK(K.zl2.reserve(2 * ncell_ml));
    HIPCHK(K.pl2.reserve(2 * ncell_ml));
  }
  HIPCHK(K.ml_mono.reserve(1));
  HIPCHK(K.wind.reserve(6 * ncell));
  HIPCHK(K.temp.reserve(2 * ncell));
  if (P.meso)
    HIPCHK(K.meso.reserve(meso_table_floats(ctx)));
  HIPCHK(K.cp2.reserve(ncol));
  HIPCHK(K.sfa.reserve(ncol));
  HIPCHK(K.sfb.reserve(2 * ncol));
  HIPCHK(K.sfc.reserve(2 * ncol));
  if (P.cloud)
    HIPCHK(K.cloud.reserve(2 * ncell));
  if (P.mx)
    HIPCHK(K.mx.reserve(2 * ncell));
  if (P.mx2)
    HIPCHK(K.mx2.reserve(7 * ncol));
  if (P.pbl) {
    HIPCHK(K.sfd.reserve(2 * ncol));
    HIPCHK(K.h2o.reserve(2 * ncell));
  }
  return 0;
}

// the table of set K from its wind records, on `stream` (K.meso allocated; no allocation, no use of ctx->err)
int meso_table_launch(const mphip_ctx *ctx, mphip_ctx::PackedGrids &K, hipStream_t stream) {
  MesoTableArgs a;
  a.wind = K.wind.p;
  a.meso = K.meso.p;
  a.nx = ctx->nx;
  a.ny = ctx->ny;
  a.np = ctx->npl;
  a.ntx = (ctx->nx + 2) / 4;
  a.nty = (ctx->ny + 2) / 4;
  hipLaunchKernelGGL(meso_table_kernel, dim3(grid_for((long long) (meso_table_floats(ctx) / 3))), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess)
    return 1;
  K.meso_valid = true;
  return 0;
}

// build the packed set K from the staging copies of two snapshots on `stream` (arrays allocated: pack_alloc).
// No allocation, no use of ctx->err: also called by the uploader thread.  *mono_pending: the monotonicity flag of
// the height columns has to be read back after the kernel (pack_finish).
int pack_launch(mphip_ctx *ctx, mphip_ctx::PackedGrids &K, const PackPlan &P, const MetSlot &s0, const MetSlot &s1,
                hipStream_t stream) {
  const size_t ncell = (size_t) ctx->nx * ctx->ny * ctx->npl, ncol = (size_t) ctx->nx * ctx->ny;
  PackArgs a;
  const MetSlot *ss[2] = { &s0, &s1 };
  for (int t = 0; t < 2; t++) {
    for (int f = 0; f < MPHIP_N3D; f++)
      a.f3[t][f] = ss[t]->has3[f] ? ss[t]->f3[f].p : nullptr;
    for (int f = 0; f < MPHIP_N2D; f++)
      a.f2[t][f] = ss[t]->has2[f] ? ss[t]->f2[f].p : nullptr;
  }
  if (P.ml_heights) {
    const int one = 1;
    if (hipMemcpyAsync(K.ml_mono.p, &one, sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess)
      return 1;
  }
  a.wind = K.wind.p;
  a.temp = K.temp.p;
  a.cloud = P.cloud ? K.cloud.p : nullptr;
  a.mx = P.mx ? K.mx.p : nullptr;
  a.mx2 = P.mx2 ? K.mx2.p : nullptr;
  a.sfa = K.sfa.p;
  a.sfb = K.sfb.p;
  a.cp2 = K.cp2.p;
  a.sfc = K.sfc.p;
  a.sfd = P.pbl ? K.sfd.p : nullptr;
  a.h2o = P.pbl ? K.h2o.p : nullptr;
  a.mlw = P.ml ? K.mlw.p : nullptr;
  a.mlw_third = P.coord2 ? MPHIP_WL : MPHIP_ZETA_DOTL;
  a.zl2 = P.ml_heights ? K.zl2.p : nullptr;
  a.pl2 = P.ml_heights ? K.pl2.p : nullptr;
  a.ml_mono = K.ml_mono.p;
  a.nml = ctx->nml;
  a.ncell = ncell;
  a.ncol = ncol;
  a.ncell_ml = (size_t) ctx->nx * ctx->ny * ctx->nml;
  K.meso_valid = false;   // (the wind records are about to change)
  hipLaunchKernelGGL(pack_kernel, dim3(grid_for((long long) ncell)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess)
    return 1;
  if (P.meso && K.meso.p && meso_table_launch(ctx, K, stream))
    return 1;
  K.ml_monotonic = false;
  if (P.ml_heights) {   // (model levels only) the fast kernel relies on monotonic height columns
    int mono = 0;
    if (hipMemcpyAsync(&mono, K.ml_mono.p, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess
        || hipStreamSynchronize(stream) != hipSuccess)
      return 1;
    K.ml_monotonic = mono != 0;
  }
  return 0;
}

// the device axes follow the current met0: after a hand-over (mphip_swap_met / mphip_commit_met) the new met0 is
// the old met1, and the reference accepts axes that differ by up to 1e-3 between files (mptrac.c:6543-6556)
int axes_follow_met0(mphip_ctx *ctx) {
  const MetSlot &s0 = ctx->slot[0 ^ ctx->flip];
  if (!s0.lon.empty() && (s0.lon != ctx->h_lon || s0.lat != ctx->h_lat || s0.p != ctx->h_p)) {
    ctx->h_lon = s0.lon;
    ctx->h_lat = s0.lat;
    ctx->h_p = s0.p;
    if (upload_axes(ctx))
      return 1;
  }
  return 0;
}

// (re)build the packed two-snapshot grids from the per-slot staging copies
int ensure_packed(mphip_ctx *ctx) {
  if (!ctx->packed_dirty)
    return 0;
  const MetSlot &s0 = ctx->slot[0 ^ ctx->flip], &s1 = ctx->slot[1 ^ ctx->flip];
  if (!s0.valid || !s1.valid)
    return fail(ctx, "meteo data for both met0 and met1 must be uploaded before stepping");
  if (axes_follow_met0(ctx))
    return 1;
  const PackPlan P = pack_plan(ctx, s0, s1);
  if (pack_alloc(ctx, ctx->pk, P))
    return 1;
  if (pack_launch(ctx, ctx->pk, P, s0, s1, ctx->stream))
    return fail(ctx, "packing the meteo grids failed");
  ctx->packed_dirty = false;
  return 0;
}

// both snapshots of the current pair are uploaded and have every 3-D field of mask3 and every 2-D field of mask2
// (bit f: field f)
bool both_have(const mphip_ctx *c, unsigned mask3, unsigned mask2 = 0) {
  const MetSlot &s0 = c->slot[0], &s1 = c->slot[1];
  bool have = s0.valid && s1.valid;
  for (int f = 0; f < MPHIP_N3D; f++)
    have = have && (!((mask3 >> f) & 1u) || (s0.has3[f] && s1.has3[f]));
  for (int f = 0; f < MPHIP_N2D; f++)
    have = have && (!((mask2 >> f) & 1u) || (s0.has2[f] && s1.has2[f]));
  return have;
}

// cache->iso_var lives on the device only while an isosurface mode needs it
int ensure_iso(mphip_ctx *ctx) {
  if (ctx->d_iso.p)
    return 0;
  const size_t n = (size_t) std::max<long long>(ctx->np, 1);
  HIPCHK(ctx->d_iso.resize(n));
  HIPCHK(ctx->d_iso_alt.resize(n));
  HIPCHK(hipMemsetAsync(ctx->d_iso.p, 0, n * sizeof(double), ctx->stream));   // calloc'ed cache_t
  return 0;
}

// every field a module mask reads must have been uploaded for both snapshots
int check_fields(mphip_ctx *ctx, unsigned mask) {
  const mphip_ctl_t &c = ctx->ctl;
  auto need3 = [&](int f, const char *who) {
    return both_have(ctx, 1u << f) ? 0 : fail(ctx, std::string(who) + ": a required 3-D meteo field was not uploaded");
  };
  auto need2 = [&](int f, const char *who) {
    return both_have(ctx, 0, 1u << f) ? 0 : fail(ctx, std::string(who) + ": a required 2-D meteo field was not uploaded");
  };
  if (mask & (MPHIP_MOD_POSITION | MPHIP_MOD_POSITION2))
    if (need2(MPHIP_PS, "module_position"))
      return 1;
  const bool model_levels = (c.advect_vert_coord == 1 || c.advect_vert_coord == 3);
  if ((mask & MPHIP_MOD_ADVECT) && c.advect_vert_coord == 2)
    if (need3(MPHIP_PL, "module_advect") || need3(MPHIP_UL, "module_advect") || need3(MPHIP_VL, "module_advect")
        || need3(MPHIP_WL, "module_advect") || ctx->nml < 2)
      return 1;
  if ((mask & MPHIP_MOD_DIFF_MESO) || ((mask & MPHIP_MOD_ADVECT) && c.advect_vert_coord == 0))
    if (need3(MPHIP_U, "module_advect") || need3(MPHIP_V, "module_advect") || need3(MPHIP_W, "module_advect"))
      return 1;
  if (((mask & MPHIP_MOD_ADVECT) && model_levels) || (mask & MPHIP_MOD_ADVECT_INIT)) {
    if (need3(MPHIP_PL, "module_advect") || need3(MPHIP_ZETAL, "module_advect")
        || need3(MPHIP_UL, "module_advect") || need3(MPHIP_VL, "module_advect")
        || need3(MPHIP_ZETA_DOTL, "module_advect") || ctx->nml < 2)
      return 1;
    if ((c.advect_vert_coord == 3 ? c.qnt_eta : c.qnt_zeta) < 0)
      return fail(ctx, "model-level advection needs quantity zeta (ADVECT_VERT_COORD 1) or eta (3)");
  }
  if (mask & MPHIP_MOD_DIFF_TURB)
    if (need2(MPHIP_PS, "module_diff_turb") || need2(MPHIP_PBL, "module_diff_turb"))
      return 1;
  if (mask & MPHIP_MOD_DIFF_PBL)
    if (need2(MPHIP_PS, "module_diff_pbl") || need2(MPHIP_PBL, "module_diff_pbl")
        || need2(MPHIP_ESS, "module_diff_pbl") || need2(MPHIP_NSS, "module_diff_pbl")
        || need2(MPHIP_SHF, "module_diff_pbl") || need3(MPHIP_T, "module_diff_pbl")
        || need3(MPHIP_H2O, "module_diff_pbl"))
      return 1;
  if (mask & MPHIP_MOD_CONVECTION) {
    if (need2(MPHIP_PS, "module_convection") || need3(MPHIP_T, "module_convection"))
      return 1;
    if (c.conv_mix_pbl && need2(MPHIP_PBL, "module_convection"))
      return 1;
    if (c.conv_cape >= 0
        && (need2(MPHIP_CAPE, "module_convection") || need2(MPHIP_CIN, "module_convection")
            || need2(MPHIP_PEL, "module_convection")))
      return 1;
  }
  if (mask & MPHIP_MOD_SEDI) {
    if (need3(MPHIP_T, "module_sedi"))
      return 1;
    if (c.qnt_rp < 0 || c.qnt_rhop < 0)
      return fail(ctx, "module_sedi needs quantities rp and rhop");
  }
  if (mask & (MPHIP_MOD_DECAY | MPHIP_MOD_WET_DEPO | MPHIP_MOD_DRY_DEPO))
    if (c.qnt_m < 0 && c.qnt_vmr < 0)
      return fail(ctx, "Module needs quantity mass or volume mixing ratio!");
  if (mask & MPHIP_MOD_WET_DEPO) {
    if (need2(MPHIP_PCT, "module_wet_depo") || need2(MPHIP_PCB, "module_wet_depo") || need2(MPHIP_CL, "module_wet_depo")
        || need3(MPHIP_T, "module_wet_depo") || need3(MPHIP_LWC, "module_wet_depo")
        || need3(MPHIP_RWC, "module_wet_depo") || need3(MPHIP_IWC, "module_wet_depo")
        || need3(MPHIP_SWC, "module_wet_depo"))
      return fail(ctx, "module_wet_depo: cloud fields (pct, pcb, cl, lwc, rwc, iwc, swc, t) were not uploaded");
  }
  if (mask & MPHIP_MOD_DRY_DEPO)
    if (need2(MPHIP_PS, "module_dry_depo"))
      return 1;
  if (mask & (MPHIP_MOD_ISOSURF | MPHIP_MOD_ISOSURF_INIT)) {
    if (c.isosurf < 1 || c.isosurf > 4)
      return fail(ctx, "module_isosurf: ISOSURF must be 1 ... 4");
    if ((c.isosurf == 2 || c.isosurf == 3) && need3(MPHIP_T, "module_isosurf"))
      return 1;
    if (c.isosurf == 4 && (mask & MPHIP_MOD_ISOSURF) && ctx->iso_n < 1)
      return fail(ctx, "module_isosurf: the balloon pressure time series was not uploaded");
    if (c.isosurf <= 3 && ensure_iso(ctx))
      return 1;
  }
  if (mask & kBound) {
    if ((c.bound_dps > 0 || c.bound_dzs > 0 || c.bound_zetas > 0 || c.bound_pbl) && need2(MPHIP_PS, "module_bound_cond"))
      return 1;
    if (c.bound_zetas > 0 && need3(MPHIP_T, "module_bound_cond"))
      return 1;
    if (c.bound_pbl && need2(MPHIP_PBL, "module_bound_cond"))
      return 1;
  }
  if ((mask & (MPHIP_MOD_DIFF_TURB | MPHIP_MOD_DECAY)) && !ctx->have_clim)
    return fail(ctx, "climatological tropopause data were not uploaded");
  return 0;
}

// The lean instantiations need a lat/lon grid with the pressure look-up table; cell indices are built with 24-bit
// multiplies (cell32: columns below 2^24, cells below 2^32).  lean32_ok: 32-bit byte offsets into the packed grids
// (the largest record has 24 bytes); lean64_ok: a grid beyond that -- or the option "big_grid" -- takes the kBigGrid
// instantiations with 64-bit offsets.
// With winds from the model levels (ADVECT_VERT_COORD 1..3) the lean kernels index the model-level records -- nml
// levels per column, which need not be the np pressure levels of the same file (met_t::npl vs met_t::np,
// mptrac.h:3862) -- so every size test takes the larger of the two level counts.
static bool ml_winds(const mphip_ctl_t &c) {   // winds from the model levels
  return c.advect_vert_coord >= 1 && c.advect_vert_coord <= 3;
}
static unsigned long long guard_levels(const mphip_ctx *ctx) {
  return (unsigned long long) (ml_winds(ctx->ctl) ? std::max(ctx->npl, ctx->nml) : ctx->npl);
}
static bool lean_grid(const mphip_ctx *ctx) {
  const unsigned long long cols = (unsigned long long) ctx->nx * ctx->ny;
  return ctx->coord_type == 0 && ctx->lut_size > 0 && cols < (1ull << 24)
    && cols * guard_levels(ctx) < (1ull << 32);
}
static bool fits32(const mphip_ctx *ctx) {
  // (the table of module_diff_meso's deviations rounds its bricks up: on a thin grid it can be the largest array)
  return (unsigned long long) ctx->nx * ctx->ny * guard_levels(ctx) * 24ull < (1ull << 32)
    && (unsigned long long) meso_table_floats(ctx) * 4ull < (1ull << 32);
}
static bool lean32_ok(const mphip_ctx *ctx) { return lean_grid(ctx) && fits32(ctx) && !ctx->big_grid; }
static bool lean64_ok(const mphip_ctx *ctx) { return lean_grid(ctx) && (!fits32(ctx) || ctx->big_grid); }

// the logical blocks of a per-particle launch with at most about `blocks` of them: per_block a multiple of 256,
// nblocks_logical a multiple of 8 (the kernels' block_range)
struct BlockGeom {
  int nblocks_logical;
  long long per_block;
};

BlockGeom block_geom(long long np, int blocks) {
  long long per_block = (np + blocks - 1) / blocks;
  per_block = std::max<long long>(256, (per_block + 255) / 256 * 256);
  const int nb = (int) ((np + per_block - 1) / per_block);
  return { (nb + 7) & ~7, per_block };
}

// the base counters of a launch's module_rng calls (StepParams::ctr_*; 0 for a module the launch does not run)
struct RngCtr {
  uint64_t turb = 0, pbl = 0, meso = 0, conv = 0;
};

// the module_rng calls of one time step of module set `mask`, counted from `base` in the reference's order:
// module_diff_turb (mptrac.c:4600, 5812), module_diff_pbl (mptrac.c:4354) and module_diff_meso take 3 np + 1 counters
// each (module_rng(..., 3 * np, 1)), module_convection np + 1 (module_rng(..., np, 0), mptrac.c:4113); *per_step: the
// counters the step takes in all
RngCtr rng_counters(unsigned mask, uint64_t np, uint64_t base, uint64_t *per_step) {
  RngCtr r;
  uint64_t next = base;
  const uint64_t triple = 3 * np + 1;
  auto take = [&](unsigned bit, uint64_t draws, uint64_t &ctr) {
    if (mask & bit) {
      ctr = next;
      next += draws;
    }
  };
  take(MPHIP_MOD_DIFF_TURB, triple, r.turb);
  take(MPHIP_MOD_DIFF_PBL, triple, r.pbl);
  take(MPHIP_MOD_DIFF_MESO, triple, r.meso);
  take(MPHIP_MOD_CONVECTION, np + 1, r.conv);
  *per_step = next - base;
  return r;
}

constexpr unsigned kNoStepKernel = 0;   // (no step_kernel instantiation has the template mask 0)

// The step_kernel instantiation of a launch of module set `mask` with nsteps time steps per particle: a lean template
// mask (before launch_step's variants of it: depo_kernel, kEmitKeys, the LDS tile), one of the general masks, or
// kNoStepKernel -- several steps per launch, and no instantiation for them.  No side effects; model-level winds read
// the packed grids' ml_monotonic (ensure_packed first).
unsigned step_kernel_mask(const mphip_ctx *ctx, unsigned mask, int nsteps) {
  const bool ml = ml_winds(ctx->ctl), fg = ctx->force_generic;
  // model levels: the fast path needs monotonic height columns and none of the rarely used modules; module_bound_cond
  // is no obstacle where the gated lean model-level instantiation can run (it switches the module at run time, as
  // every gated instantiation does)
  const bool ml_cols = ml && ctx->pk.ml_monotonic && ctx->nml <= kLockstepMaxLevels && !fg;
  const bool ml_fast = ml_cols && !(mask & (kRareModules & ~MPHIP_MOD_ADVECT_INIT));
  const bool ml_fast_bound = ml_cols && !(mask & (kRareModules & ~MPHIP_MOD_ADVECT_INIT & ~kBound));
  const unsigned rare_bits = mask & kRareModules & ~(ml_fast ? MPHIP_MOD_ADVECT_INIT : 0u);
  // the lean instantiations run a lat/lon grid with a pressure look-up table, and take module_timesteps / the dt store
  // from the run-time mask; they are keyed on the movers (loss / decay / deposition are run-time bits in all of them)
  const bool lean_ok = !fg && lean32_ok(ctx), big_ok = !fg && lean64_ok(ctx);
  const unsigned req = (mask | MPHIP_MOD_TIMESTEPS) & ~(kStoreDt | kTailModules | kBound);
  const unsigned multi = nsteps > 1 ? kMultiStep : 0u;
  // (ADVECT 2 and 1 -- midpoint, the reference's default, and Euler -- share the two-stage instantiations)
  const unsigned scheme = (mask & MPHIP_MOD_ADVECT) && ctx->ctl.advect != 4 ? kTwoStage : 0u;
  // An exact module set has its own lean instantiation.  Any other subset of {turbulent, mesoscale diffusion,
  // convection, sedimentation} on top of the time step's movers, and every set with module_bound_cond, runs the
  // largest one with those switched at run time (kGated; module_bound_cond also in the instantiation without
  // movers).  Everything else (single-module calls, the other rarely used modules) takes a general instantiation.
  constexpr unsigned kClosure = MPHIP_MOD_DIFF_PBL | MPHIP_MOD_ISOSURF;
  unsigned sel = kNoStepKernel;
  if (ml) {
    // model-level winds: the headline module set has lean instantiations (its subsets the gated one); the rest
    // stays with the general model-level kernels below
    if (!(rare_bits & ~kBound) && (ml_fast || (ml_fast_bound && (mask & kBound))) && (lean_ok || big_ok)) {
      if (req == kAdvDiffConvSedi && !(mask & kBound) && lean_ok)
        sel = req | kMLWinds | multi;
      else if ((req & ~kOptionalModules) == kAdv)   // (subsets, every set with module_bound_cond, and every set of a big grid)
        sel = kAdvDiffConvSedi | kGated | kMLWinds | (big_ok ? kBigGrid : 0u) | multi;
    }
  } else if (mask & kClosure) {
    // the closure inside the boundary layer (TURB_PBL_SCHEME 1) and module_isosurf: gated instantiations of their own
    if (!(rare_bits & ~(kBound | kClosure)) && lean_ok && ((req & ~kClosure & ~kOptionalModules) == kAdv))
      sel = kAdvDiffConvSedi | kGated | kPblClosure | scheme | multi;
  } else if (!(rare_bits & ~kBound) && lean_ok) {
    // (kAdvTurbConvSedi has a kernel of its own for single steps only: several steps per launch take the gated one)
    const bool exact = req == kAdv || req == kAdvTurb || req == kAdvDiff || req == kAdvDiffConvSedi
      || (req == kAdvTurbConvSedi && nsteps == 1);
    if (req == kTailOnly)
      sel = kTailOnly;
    else if (req == kDiffConvSediOnly && !(mask & kBound))
      sel = kDiffConvSediOnly;
    else if (exact && !(mask & kBound))
      sel = req | scheme | multi;
    else if ((req & ~kOptionalModules) == kAdv)
      sel = kAdvDiffConvSedi | kGated | scheme | multi;
  } else if (!(rare_bits & ~kBound) && big_ok && (req & ~kOptionalModules) == kAdv) {
    // a grid beyond 32-bit offsets: the gated instantiation with 64-bit ones serves every set of the time step's movers
    sel = kAdvDiffConvSedi | kGated | kBigGrid | scheme | multi;
  }
#ifdef MPHIP_QUICK   // (a development build with the five instantiations the headline workloads launch -- the fifth is
                     // kAdvDiffConvSedi's kEmitKeys variant; every other module set runs a general kernel)
  if (sel != kAdvDiffConvSedi && sel != (kAdvDiffConvSedi | kMultiStep) && sel != (kAdvDiffConvSedi | kMLWinds | kMultiStep)
      && sel != (kAdvDiffConvSedi | kGated | kPblClosure | kMultiStep))
    sel = kNoStepKernel;
#endif
  if (sel != kNoStepKernel)
    return sel;
  if (ml_fast)
    return nsteps > 1 ? kMaskGenericMLMulti : kMaskGenericML;
  if (nsteps > 1)
    return kNoStepKernel;
  return ml || (mask & kRareModules) || fg ? kMaskGeneric : kMaskGenericPL;
}

// Does instantiation `sel`, launched with module set `mask`, read the table of module_diff_meso's wind deviations?  The
// lean instantiations with 32-bit offsets do (diff_meso_fast); the gated ones switch the module by the run-time mask.
static bool reads_meso_table(unsigned sel, unsigned mask) {
  return sel != kNoStepKernel && sel < kMaskGenericMLMulti && (sel & MPHIP_MOD_DIFF_MESO)
    && !(sel & kBigGrid) && (mask & MPHIP_MOD_DIFF_MESO);
}

// the table of the current packed set, for a launch that reads it: built with the set (pack_launch) where the module
// was on then; otherwise here, in front of the first such launch (the one place that may have to allocate it)
int ensure_meso_table(mphip_ctx *ctx) {
  mphip_ctx::PackedGrids &K = ctx->pk;
  if (K.meso_valid)
    return 0;
  HIPCHK(K.meso.reserve(meso_table_floats(ctx)));
  if (meso_table_launch(ctx, K, ctx->stream))
    return fail(ctx, "building the table of the mesoscale wind deviations failed");
  return 0;
}

// The chunk queues of a step_kernel launch (option step_queue; the kernel's chunk_claim).  The grid is what the GPU
// holds at a time -- the workgroups of this instantiation with this much dynamic LDS per CU, asked once per context,
// times the CUs -- or the option's bound `blocks` (step_blocks, step_blocks_multi) if that is less, a multiple of 8:
// every workgroup fills its LDS tables once and its waves then claim chunks until none is left, so the launch ends
// within one chunk's time of its last wave, not one block's.  The queues have a price per launch that does not depend
// on the particle count: at its end every wave finds up to eight queues used up and adds to the counter of finished
// waves, 4 096 waves x 9 returning atomics on nine words, 30-50 us measured (C3 at 10^6 particles, one launch per step:
// 0.194 -> 0.224 ms; C2: 0.078 -> 0.130 ms; at 10^7 particles the same launches gain 0.07 ms,
// profiles/r10_step_queue_ab.txt).  So step_queue 1 takes them from kQueueChunksPerWave chunks per wave of the grid on
// -- 65 536 chunks, 4.2 million particles, at 256 CUs with four workgroups each -- and keeps the static partition
// below; between 10^6 and 10^7 particles nothing was measured.  Fills S.queue* and *grid; leaves both alone where the
// static partition stays.
constexpr int kQueueChunksPerWave = 16;
int step_queue_grid(mphip_ctx *ctx, void (*kernel)(const StepParams), size_t lds, int blocks, StepParams &S, int *grid) {
  if (ctx->step_queue == 0)
    return 0;
  const auto key = std::make_pair((const void *) kernel, lds);
  auto it = ctx->step_resident.find(key);
  if (it == ctx->step_resident.end()) {
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    it = ctx->step_resident.emplace(key, std::max(per_cu, 1) * std::max(cus, 1)).first;
  }
  const long long nchunks = (ctx->np + 63) / 64;
  long long g = std::max<long long>(8, std::min(it->second, blocks) & ~7);
  if (nchunks > 0x7fffffffll || (ctx->step_queue == 1 && nchunks < (long long) kQueueChunksPerWave * kStepWaves * g))
    return 0;
  g = std::min(g, ((nchunks + kStepWaves - 1) / kStepWaves + 7) & ~7ll);   // (no more waves than chunks, in whole eights)
  if (!ctx->d_step_queue.p) {
    HIPCHK(ctx->d_step_queue.resize(kQueueInts));
    HIPCHK(hipMemsetAsync(ctx->d_step_queue.p, 0, kQueueInts * sizeof(int), ctx->stream));
  }
  S.queue = ctx->d_step_queue.p;
  S.queue_n = ctx->xcd_map ? 8 : 1;
  S.queue_chunks = (int) ((nchunks + S.queue_n - 1) / S.queue_n);
  S.queue_waves = (int) g * kStepWaves;
  *grid = (int) g;
  return 0;
}

// nsteps > 1: that many consecutive time steps in one launch, time and counters advancing by t_stride and ctr_stride
// (kMultiStep instantiations: step_kernel_mask says whether one exists for the module set)
int launch_step(mphip_ctx *ctx, unsigned mask, double t, const RngCtr &rng = {}, int nsteps = 1, double t_stride = 0,
                uint64_t ctr_stride = 0, const EmitKeys *emit = nullptr, bool *emitted = nullptr) {
  if (ctx->np == 0)
    return 0;
  if (ensure_packed(ctx) || check_fields(ctx, mask))
    return 1;
  if (ml_winds(ctx->ctl) && !ctx->d_kz.p) {
    const size_t n = (size_t) std::max<long long>(ctx->np, 1);
    HIPCHK(ctx->d_kz.resize(n));
    HIPCHK(ctx->d_kz_alt.resize(n));
    std::vector<int> mid(n, std::max(ctx->nml / 2, 0));     // any level: the hint only shortens the search
    HIPCHK(hipMemcpyAsync(ctx->d_kz.p, mid.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  StepParams S;
  memset(&S.emit, 0, sizeof(S.emit));
  S.depo_busy = nullptr;
  if (emitted)
    *emitted = false;
  S.ctl = ctx->ctl;
  S.met = dev_met(ctx);
  S.atm = dev_atm(ctx);
  S.clim = ctx->d_clim.p;
  S.tracers = ctx->d_tracers.p;
  S.t = t;
  S.mask = mask;
  // The static partition (step_queue 0, launches below step_queue_grid's threshold, and the kernels other than
  // step_kernel): every block walks a whole number of 256-particle rounds (no half-empty last round).  block_geom
  // rounds per_block up to a multiple of 256, so the option is an upper bound: 10^7 particles make 7 813 blocks of 1 280
  // under step_blocks 8 192, and 19 532 blocks of 512 under step_blocks_multi 32 768.
  // (multi-step launches: more, shorter blocks -- a launch ends one block's time after its last block starts, and a
  // block that takes 20 steps per particle lasts long; measured on C3 at 20 steps per launch, alternating in one
  // process: 0.744-0.781 / 0.738-0.757 / 0.729-0.747 ms per step with bounds of 8 192 / 16 384 / 32 768 blocks)
  const BlockGeom geom = block_geom(ctx->np, nsteps > 1 ? ctx->step_blocks_multi : ctx->step_blocks);
  const int nb = geom.nblocks_logical;
  const long long per_block = geom.per_block;
  S.nblocks_logical = nb;
  S.per_block = per_block;
  S.xcd_map = ctx->xcd_map;
  S.ctr_turb = rng.turb;
  S.ctr_meso = rng.meso;
  S.ctr_conv = rng.conv;
  S.ctr_pbl = rng.pbl;
  S.radio = ctx->radio;
  S.nsteps = nsteps;
  S.t_stride = t_stride;
  S.ctr_stride = ctr_stride;
  S.queue = nullptr;   // (the static partition; step_queue_grid below)
  S.queue_n = S.queue_chunks = S.queue_waves = 0;
  // axes, climatological tropopause, the tables of log and exp (+ pow's for the instantiations with the closure, below)
  size_t lds = axes_lds_bytes(ctx) + sizeof(DevClim) + (size_t) kLibmLogExpDoubles * sizeof(double);
  hipEvent_t e1 = nullptr;
  if (prof_pair(ctx, ctx->stream, &e1))
    return 1;
  unsigned sel = step_kernel_mask(ctx, mask, nsteps);
  if (reads_meso_table(sel, mask)) {
    if (ensure_meso_table(ctx))
      return 1;
    S.met.meso = ctx->pk.meso.p;
  }
  // module_wet_depo / module_dry_depo alone (the launch behind module_mixing): the kernel that packs the few
  // particles with anything to do into full waves
  constexpr unsigned kDepo = MPHIP_MOD_WET_DEPO | MPHIP_MOD_DRY_DEPO;
  const size_t depo_lds = ((axes_lds_bytes(ctx) + 15) & ~(size_t) 15) + (size_t) per_block * sizeof(int);
  if (sel == kTailOnly && (mask & kDepo) && !(mask & ~kDepo) && ctx->compact_depo && !ctx->fused_perm
      && depo_lds <= 64 * 1024) {
    S.depo_busy = ctx->depo_busy_valid ? ctx->d_depo_busy.p : nullptr;
    ctx->depo_busy_valid = false;
    ctx->depo_busy_last = S.depo_busy;      // (module_radio_depo behind this launch looks at the same particles)
    ctx->depo_busy_last_mask = mask;
    hipLaunchKernelGGL(depo_kernel, dim3(nb), dim3(256), depo_lds, ctx->stream, S);
    HIPCHK(hipGetLastError());
    ctx->fused_perm = nullptr;
    if (ctx->prof)
      HIPCHK(hipEventRecord(e1, ctx->stream));
    return 0;
  }
  // the headline module set, one step per launch, and the caller wants the keys of the sort ahead from this launch
  ctx->depo_busy_valid = false;     // (any other launch: positions may move, the flags of an earlier one are void)
  ctx->depo_busy_last = nullptr;
  if (emit && emit->keys && sel == kAdvDiffConvSedi && nsteps == 1) {
    sel |= kEmitKeys;
    S.emit = *emit;
    if (emitted)
      *emitted = true;
    ctx->depo_busy_valid = emit->depo_busy != nullptr;
  }
  // pure trajectories, several steps per launch: the kernel that stages the wind grid through an LDS tile (option lds_tile)
  if (ctx->lds_tile > 0 && nsteps > 1 && (sel == (kAdv | kMultiStep) || sel == (kAdv | kTwoStage | kMultiStep))
      && !(mask & (kTailModules | kBound)) && !ctx->fused_perm) {
    const size_t tile_lds = ((axes_lds_bytes(ctx) + 15) & ~(size_t) 15) + (size_t) ctx->lds_tile * 24;
    if (tile_lds <= 64 * 1024) {
      if (sel & kTwoStage)
        hipLaunchKernelGGL(traj_tile_kernel<2>, dim3(nb), dim3(256), tile_lds, ctx->stream, S, ctx->lds_tile);
      else
        hipLaunchKernelGGL(traj_tile_kernel<4>, dim3(nb), dim3(256), tile_lds, ctx->stream, S, ctx->lds_tile);
      HIPCHK(hipGetLastError());
      if (ctx->prof)
        HIPCHK(hipEventRecord(e1, ctx->stream));
      return 0;
    }
  }
  if (sel < kMaskGenericMLMulti && (sel & kPblClosure))
    lds += (size_t) (kLibmDoubles - kLibmLogExpDoubles) * sizeof(double);
  if (step_kernel_parks(sel))   // + the thread-private parking area in front of them (step_kernel: park_slot)
    lds += kParkBytes;
  // (-DMPHIP_QUICK: only the instantiations step_kernel_mask selects in that build)
  void (*kernel)(const StepParams) = nullptr;
  switch (sel) {
#define STEP_CASE(M)                                                                                  \
  case M:                                                                                             \
    kernel = step_kernel<M>;                                                                          \
    break;
#ifdef MPHIP_QUICK
#define STEP_CASE_REST(M)
#else
#define STEP_CASE_REST(M) STEP_CASE(M)
#endif
    STEP_CASE_REST(kAdv)
    STEP_CASE_REST(kAdvTurb)
    STEP_CASE_REST(kAdvDiff)
    STEP_CASE_REST(kAdvTurbConvSedi)
    STEP_CASE(kAdvDiffConvSedi)
    STEP_CASE_REST(kAdv | kTwoStage)
    STEP_CASE_REST(kAdvTurb | kTwoStage)
    STEP_CASE_REST(kAdvDiff | kTwoStage)
    STEP_CASE_REST(kAdvTurbConvSedi | kTwoStage)
    STEP_CASE_REST(kAdvDiffConvSedi | kTwoStage)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kTwoStage)
    STEP_CASE_REST(kTailOnly)
    STEP_CASE_REST(kDiffConvSediOnly)
    STEP_CASE_REST(kAdv | kMultiStep)
    STEP_CASE_REST(kAdvTurb | kMultiStep)
    STEP_CASE_REST(kAdvDiff | kMultiStep)
    STEP_CASE(kAdvDiffConvSedi | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kMLWinds)
    STEP_CASE(kAdvDiffConvSedi | kMLWinds | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kMLWinds)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kMLWinds | kMultiStep)
    STEP_CASE_REST(kAdv | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvTurb | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvDiff | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kTwoStage | kMultiStep)
    STEP_CASE(kAdvDiffConvSedi | kEmitKeys)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kPblClosure)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kPblClosure | kTwoStage)
    STEP_CASE(kAdvDiffConvSedi | kGated | kPblClosure | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kPblClosure | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid | kTwoStage)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid | kTwoStage | kMultiStep)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid | kMLWinds)
    STEP_CASE_REST(kAdvDiffConvSedi | kGated | kBigGrid | kMLWinds | kMultiStep)
    STEP_CASE(kMaskGeneric)
    STEP_CASE(kMaskGenericMLMulti)
    STEP_CASE(kMaskGenericML)
    STEP_CASE(kMaskGenericPL)
#undef STEP_CASE_REST
#undef STEP_CASE
  default:   // kNoStepKernel
    return fail(ctx, "internal: no multi-step instantiation for this module set");
  }
  int grid = nb;
  if (step_queue_grid(ctx, kernel, lds, nsteps > 1 ? ctx->step_blocks_multi : ctx->step_blocks, S, &grid))
    return 1;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, ctx->stream, S);
  HIPCHK(hipGetLastError());
  ctx->fused_perm = nullptr;   // module_sort's gather, if one was pending, has happened in this launch
  if (ctx->prof)
    HIPCHK(hipEventRecord(e1, ctx->stream));
  return 0;
}

// ---- module_meteo -------------------------------------------------------------

// meteo fields each module_meteo quantity is computed from (mptrac.c:5091-5157)
struct MeteoDeps {
  unsigned need3 = 0, need2 = 0;
};

MeteoDeps meteo_deps(const mphip_ctl_t &c) {
  MeteoDeps d;
  auto q = [&](int k) { return c.qnt_met[k] >= 0; };
  auto f3 = [&](int k, int f) { if (q(k)) d.need3 |= 1u << f; };
  auto f2 = [&](int k, int f) { if (q(k)) d.need2 |= 1u << f; };
  f2(MPHIP_MQ_PS, MPHIP_PS);     f2(MPHIP_MQ_TS, MPHIP_TS);     f2(MPHIP_MQ_ZS, MPHIP_ZS);
  f2(MPHIP_MQ_US, MPHIP_US);     f2(MPHIP_MQ_VS, MPHIP_VS);     f2(MPHIP_MQ_ESS, MPHIP_ESS);
  f2(MPHIP_MQ_NSS, MPHIP_NSS);   f2(MPHIP_MQ_SHF, MPHIP_SHF);   f2(MPHIP_MQ_LSM, MPHIP_LSM);
  f2(MPHIP_MQ_SST, MPHIP_SST);   f2(MPHIP_MQ_PBL, MPHIP_PBL);   f2(MPHIP_MQ_PT, MPHIP_PT);
  f2(MPHIP_MQ_TT, MPHIP_TT);     f2(MPHIP_MQ_ZT, MPHIP_ZT);     f2(MPHIP_MQ_H2OT, MPHIP_H2OT);
  f2(MPHIP_MQ_PCT, MPHIP_PCT);   f2(MPHIP_MQ_PCB, MPHIP_PCB);   f2(MPHIP_MQ_CL, MPHIP_CL);
  f2(MPHIP_MQ_PLCL, MPHIP_PLCL); f2(MPHIP_MQ_PLFC, MPHIP_PLFC); f2(MPHIP_MQ_PEL, MPHIP_PEL);
  f2(MPHIP_MQ_CAPE, MPHIP_CAPE); f2(MPHIP_MQ_CIN, MPHIP_CIN);   f2(MPHIP_MQ_O3C, MPHIP_O3C);
  f3(MPHIP_MQ_ZG, MPHIP_Z);      f3(MPHIP_MQ_T, MPHIP_T);       f3(MPHIP_MQ_U, MPHIP_U);
  f3(MPHIP_MQ_V, MPHIP_V);       f3(MPHIP_MQ_W, MPHIP_W);       f3(MPHIP_MQ_H2O, MPHIP_H2O);
  f3(MPHIP_MQ_O3, MPHIP_O3);     f3(MPHIP_MQ_LWC, MPHIP_LWC);   f3(MPHIP_MQ_RWC, MPHIP_RWC);
  f3(MPHIP_MQ_IWC, MPHIP_IWC);   f3(MPHIP_MQ_SWC, MPHIP_SWC);   f3(MPHIP_MQ_CC, MPHIP_CC);
  f3(MPHIP_MQ_PV, MPHIP_PV);
  // derived quantities
  f3(MPHIP_MQ_RHO, MPHIP_T);     f3(MPHIP_MQ_VH, MPHIP_U);      f3(MPHIP_MQ_VH, MPHIP_V);
  f3(MPHIP_MQ_VZ, MPHIP_W);      f3(MPHIP_MQ_PSAT, MPHIP_T);    f3(MPHIP_MQ_PSICE, MPHIP_T);
  f3(MPHIP_MQ_PW, MPHIP_H2O);    f3(MPHIP_MQ_SH, MPHIP_H2O);    f3(MPHIP_MQ_RH, MPHIP_T);
  f3(MPHIP_MQ_RH, MPHIP_H2O);    f3(MPHIP_MQ_RHICE, MPHIP_T);   f3(MPHIP_MQ_RHICE, MPHIP_H2O);
  f3(MPHIP_MQ_THETA, MPHIP_T);   f3(MPHIP_MQ_ZETA_D, MPHIP_T);  f2(MPHIP_MQ_ZETA_D, MPHIP_PS);
  f3(MPHIP_MQ_TVIRT, MPHIP_T);   f3(MPHIP_MQ_TVIRT, MPHIP_H2O); f3(MPHIP_MQ_LAPSE, MPHIP_T);
  f3(MPHIP_MQ_LAPSE, MPHIP_H2O); f3(MPHIP_MQ_TDEW, MPHIP_H2O);  f3(MPHIP_MQ_TICE, MPHIP_H2O);
  f3(MPHIP_MQ_TNAT, MPHIP_H2O);
  return d;
}

bool meteo_requested(const mphip_ctl_t &c) {
  for (int k = 0; k < MPHIP_NMQ; k++)
    if (c.qnt_met[k] >= 0)
      return true;
  return false;
}

// checks of a module_meteo call (quantity indices, uploaded fields); 0 = fine
int check_meteo(mphip_ctx *ctx) {
  const mphip_ctl_t &c = ctx->ctl;
  if (ctx->np == 0 || !meteo_requested(c))
    return 0;
  for (int k = 0; k < MPHIP_NMQ; k++)
    if (c.qnt_met[k] >= c.nq)
      return fail(ctx, "module_meteo: quantity index out of range");
  if (!both_have(ctx, 0))
    return fail(ctx, "meteo data for both met0 and met1 must be uploaded before stepping");
  const char *const *const n3 = kField3Name;
  static const char *const n2[MPHIP_N2D] = { "ps", "pbl", "cape", "cin", "pel", "pct", "pcb", "cl", "ess", "nss", "shf",
                                             "ts", "zs", "us", "vs", "lsm", "sst", "pt", "tt", "zt", "h2ot", "plcl",
                                             "plfc", "o3c" };
  // the climatology quantities: tables, and the rule of mptrac.c:5074-5076
  static const struct { int q, zm; const char *name; } zmq[] = {
    { MPHIP_MQ_HNO3, MPHIP_ZM_HNO3, "HNO3" }, { MPHIP_MQ_TNAT, MPHIP_ZM_HNO3, "HNO3" }, { MPHIP_MQ_OH, MPHIP_ZM_OH, "OH" },
    { MPHIP_MQ_H2O2, MPHIP_ZM_H2O2, "H2O2" }, { MPHIP_MQ_HO2, MPHIP_ZM_HO2, "HO2" }, { MPHIP_MQ_O1D, MPHIP_ZM_O1D, "O1D" } };
  for (const auto &e : zmq)
    if (c.qnt_met[e.q] >= 0 && !ctx->d_zm[e.zm].p)
      return fail(ctx, std::string("module_meteo: the ") + e.name + " climatology was not uploaded");
  if (c.qnt_met[MPHIP_MQ_TSTS] >= 0 && (c.qnt_met[MPHIP_MQ_TICE] < 0 || c.qnt_met[MPHIP_MQ_TNAT] < 0))
    return fail(ctx, "Need T_ice and T_NAT to calculate T_STS!");
  const MeteoDeps d = meteo_deps(c);
  for (int f = 0; f < MPHIP_N3D; f++)
    if (((d.need3 >> f) & 1u) && !both_have(ctx, 1u << f))
      return fail(ctx, std::string("module_meteo: meteo field ") + n3[f] + " was not uploaded");
  for (int f = 0; f < MPHIP_N2D; f++)
    if (((d.need2 >> f) & 1u) && !both_have(ctx, 0, 1u << f))
      return fail(ctx, std::string("module_meteo: meteo field ") + n2[f] + " was not uploaded");
  return 0;
}

// fields a MeteoArgs kernel needs on the current pair (masks as both_have's) and its refusal without them
struct FieldNeed {
  unsigned mask3, mask2;
  const char *refusal;
};

// a kernel over MeteoArgs on every particle (meteo_kernel, the chemistry kernels): nothing without particles; else the
// packed grids, the fields of `needs` in order, and the launch with the climatology tables of zm_mask (bit k: table k),
// the fields the kernel interpolates (`reads`: MeteoArgs::need3 / need2) and `extra` behind MeteoArgs
template <class Kernel, class... Extra>
int launch_meteo_args(mphip_ctx *ctx, Kernel kernel, std::initializer_list<FieldNeed> needs, unsigned zm_mask,
                      const MeteoDeps &reads, Extra... extra) {
  if (ctx->np == 0)
    return 0;
  if (ensure_packed(ctx))
    return 1;
  for (const FieldNeed &n : needs)
    if (!both_have(ctx, n.mask3, n.mask2))
      return fail(ctx, n.refusal);
  MeteoArgs G;
  memset(&G, 0, sizeof(G));
  G.ctl = ctx->ctl;
  G.met = dev_met(ctx);
  G.atm = dev_atm(ctx);
  G.need3 = reads.need3;
  G.need2 = reads.need2;
  for (int k = 0; k < MPHIP_NZM; k++)
    if ((zm_mask >> k) & 1u)
      G.zm[k] = ctx->zm[k];
  const BlockGeom geom = block_geom(ctx->np, ctx->step_blocks);
  G.nblocks_logical = geom.nblocks_logical;
  G.per_block = geom.per_block;
  G.xcd_map = ctx->xcd_map;
  hipLaunchKernelGGL(kernel, dim3(geom.nblocks_logical), dim3(256), axes_lds_bytes(ctx), ctx->stream, G, extra...);
  HIPCHK(hipGetLastError());
  return 0;
}

// module_oh_chem (mptrac.c:5351-5434): its own kernel, on the dt the step's launch stored (oh_chem_kernel)
int launch_oh(mphip_ctx *ctx) {
  const mphip_ctl_t &c = ctx->ctl;
  if (c.oh_chem_reaction < 1 || c.oh_chem_reaction > 3)
    return fail(ctx, "module_oh_chem: OH_CHEM_REACTION must be 1, 2 or 3");
  if (c.qnt_m < 0 && c.qnt_vmr < 0)
    return fail(ctx, "Module needs quantity mass or volume mixing ratio!");
  if (!ctx->d_zm[MPHIP_ZM_OH].p)
    return fail(ctx, "module_oh_chem: the OH climatology was not uploaded");
  return launch_meteo_args(ctx, oh_chem_kernel, { { 1u << MPHIP_T, 0, "module_oh_chem: meteo field t was not uploaded" } },
                           1u << MPHIP_ZM_OH, MeteoDeps());
}

// module_tracer_chem: its own kernel behind module_h2o2_chem, on the dt the step's launch stored (tracer_chem_kernel).
// Without a present CFC or N2O quantity it does nothing (Csf6 has no reaction).
int launch_tracer_chem(mphip_ctx *ctx) {
  const mphip_ctl_t &c = ctx->ctl;
  static const char *const names[4] = { "Cccl4", "Cccl3f", "Cccl2f2", "Cn2o" };
  bool any = false;
  for (int k = 0; k < 4; k++)
    any = any || c.qnt_tracer[k] >= 0;
  if (!any)
    return 0;
  if (c.met_coord_type != 0)
    return fail(ctx, "module_tracer_chem: not implemented for MET_COORD_TYPE != 0 (the photolysis and O(1D) tables "
                     "are on latitude and longitude)");
  if (!ctx->d_zm[MPHIP_ZM_O1D].p)
    return fail(ctx, "module_tracer_chem: the O1D climatology was not uploaded");
  for (int k = 0; k < 4; k++)
    if (c.qnt_tracer[k] >= 0 && !ctx->photo_have[k])
      return fail(ctx, std::string("module_tracer_chem: the photolysis rates of quantity ") + names[k]
                         + " were not uploaded");
  return launch_meteo_args(ctx, tracer_chem_kernel,
                           { { 1u << MPHIP_T, 0, "module_tracer_chem: meteo field t was not uploaded" },
                             { 0, 1u << MPHIP_O3C, "module_tracer_chem: meteo field o3c was not uploaded" } },
                           1u << MPHIP_ZM_O1D, MeteoDeps(), ctx->photo);
}

// module_h2o2_chem: its own kernel behind module_oh_chem, on the dt the step's launch stored (h2o2_chem_kernel)
int launch_h2o2(mphip_ctx *ctx) {
  const mphip_ctl_t &c = ctx->ctl;
  if (c.qnt_m < 0 && c.qnt_vmr < 0)
    return fail(ctx, "Module needs quantity mass or volume mixing ratio!");
  if (!ctx->d_zm[MPHIP_ZM_H2O2].p)
    return fail(ctx, "module_h2o2_chem: the H2O2 climatology was not uploaded");
  return launch_meteo_args(ctx, h2o2_chem_kernel,
                           { { 1u << MPHIP_T | 1u << MPHIP_LWC | 1u << MPHIP_RWC, 0,
                               "module_h2o2_chem: meteo fields t, lwc and rwc were not uploaded" } },
                           1u << MPHIP_ZM_H2O2, MeteoDeps(), ctx->h2o2_low);
}

int launch_meteo(mphip_ctx *ctx) {
  const mphip_ctl_t &c = ctx->ctl;
  if (ctx->np == 0 || !meteo_requested(c))
    return 0;   // nothing to set: every SET_ATM of the reference is a no-op
  if (check_meteo(ctx))
    return 1;
  return launch_meteo_args(ctx, meteo_kernel, {}, (1u << MPHIP_NZM) - 1, meteo_deps(c));
}

// module_meteo of mphip_run_timestep: checked now, run when its result can be seen (lazy_meteo)
int schedule_meteo(mphip_ctx *ctx) {
  if (!ctx->lazy_meteo)
    return launch_meteo(ctx);
  if (check_meteo(ctx))
    return 1;
  ctx->meteo_pending = true;
  return 0;
}

int flush_meteo(mphip_ctx *ctx) {
  if (!ctx->meteo_pending)
    return 0;
  ctx->meteo_pending = false;
  return launch_meteo(ctx);
}

PermGeom perm_geom(long long n) {
  PermGeom pg;
  long long per_block = (n + 8191) / 8192;
  per_block = std::max<long long>(256, (per_block + 255) / 256 * 256);
  int nb = (int) ((n + per_block - 1) / per_block);
  pg.nblocks = std::max(8, (nb + 7) & ~7);
  pg.per_block = per_block;
  return pg;
}

PermArgs perm_args(mphip_ctx *ctx, bool with_cache) {
  PermArgs g;
  memset(&g, 0, sizeof(g));
  g.n8 = 4 + ctx->nq;
  for (int k = 0; k < g.n8; k++) {
    g.in8[k] = ctx->d_arr[k].p;
    g.out8[k] = ctx->d_alt[k].p;
  }
  if (with_cache) {
    g.in8[g.n8] = ctx->d_dt.p;
    g.out8[g.n8] = ctx->d_dt_alt.p;
    g.n8++;
    if (ctx->d_iso.p) {
      g.in8[g.n8] = ctx->d_iso.p;
      g.out8[g.n8] = ctx->d_iso_alt.p;
      g.n8++;
    }
    g.n4 = 3;
    for (int k = 0; k < 3; k++) {
      g.in4[k] = ctx->d_uvwp[k].p;
      g.out4[k] = ctx->d_uvwp_alt[k].p;
    }
    if (ctx->d_kz.p) {
      g.in4[3] = (const float *) ctx->d_kz.p;
      g.out4[3] = (float *) ctx->d_kz_alt.p;
      g.n4 = 4;
    }
  }
  return g;
}

void perm_swap(mphip_ctx *ctx, bool with_cache) {
  for (int k = 0; k < 4 + ctx->nq; k++)
    std::swap(ctx->d_arr[k], ctx->d_alt[k]);
  if (with_cache) {
    std::swap(ctx->d_dt, ctx->d_dt_alt);
    std::swap(ctx->d_iso, ctx->d_iso_alt);
    std::swap(ctx->d_kz, ctx->d_kz_alt);
    for (int k = 0; k < 3; k++)
      std::swap(ctx->d_uvwp[k], ctx->d_uvwp_alt[k]);
  }
}

// stable LSD radix sort of n (key, value) pairs that starts in keys[0] / vals[0] and ping-pongs between the two
// buffer pairs; *cur_out = the pair that holds the result
// (n_dev: the number of pairs lives on the device and n is only its upper bound)
// (index_sort: the values are the positions 0, 1, 2 ...; vals[0] is not read, the first pass generates them)
// (packed_first: the input is keys[0] read as n interleaved (key, value) pairs -- 2 n words that may overlap
//  vals[0], which is then not read; the passes write to keys[1] / vals[1] first)
int radix_passes(mphip_ctx *ctx, uint32_t *const keys[2], int *const vals[2], long long n, int key_bits, int *cur_out,
                 const uint32_t *n_dev = nullptr, bool index_sort = false, bool packed_first = false) {
  *cur_out = 0;
  if (n <= 0)
    return 0;
  const int ntiles = (int) ((n + kSortTile - 1) / kSortTile);
  // digit width with the fewest passes (8 bits if it is a tie)
  int bits = ctx->sort_bits;
  if (bits == 0) {
    bits = 8;
    for (int b = 9; b <= kRadixMaxBits; b++)
      if ((key_bits + b - 1) / b < (key_bits + bits - 1) / bits)
        bits = b;
  }
  const int passes = (key_bits + bits - 1) / bits;
  const size_t m = ((size_t) 1 << bits) * ntiles;
  // chunk length of the two-level scan: 4096 counters while <= 1024 chunks cover m, else 16384
  const bool small = (m + kScanThreads * kScanPerSmall - 1) / (kScanThreads * kScanPerSmall) <= (size_t) kScanThreads;
  const int chunk_shift = small ? 12 : 14;
  static_assert(kScanThreads * kScanPerSmall == 1 << 12 && kScanThreads * kScanPerLarge == 1 << 14, "chunk lengths");
  const int nchunks = (int) ((m + ((size_t) 1 << chunk_shift) - 1) >> chunk_shift);
  if (nchunks > kScanThreads)
    return fail(ctx, "too many particles for the two-level scan of the radix sort");
  HIPCHK(ctx->d_counts.reserve(m + kScanThreads));   // counters + chunk totals
  uint32_t *d_chunks = ctx->d_counts.p + m;
  int cur = 0;
  for (int pass = 0; pass < passes; pass++) {
    const int shift = bits * pass;
    const int stride = packed_first && pass == 0 ? 2 : 1;
#define SORT_PASS(B)                                                                                                   \
  hipLaunchKernelGGL(sort_hist_kernel<B>, dim3(ntiles), dim3(kSortThreads), 0, ctx->stream, keys[cur], n, shift,       \
                     ntiles, ctx->d_counts.p, n_dev, stride);                                                            \
  if (small)                                                                                                           \
    hipLaunchKernelGGL(sort_scan_local_kernel<kScanPerSmall>, dim3(nchunks), dim3(kScanThreads), 0, ctx->stream,       \
                       ctx->d_counts.p, m, d_chunks, n_dev, 1 << B);                                                     \
  else                                                                                                                 \
    hipLaunchKernelGGL(sort_scan_local_kernel<kScanPerLarge>, dim3(nchunks), dim3(kScanThreads), 0, ctx->stream,       \
                       ctx->d_counts.p, m, d_chunks, n_dev, 1 << B);                                                     \
  hipLaunchKernelGGL(sort_scan_chunks_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_chunks, nchunks);         \
  hipLaunchKernelGGL(sort_scatter_kernel<B>, dim3(ntiles), dim3(kSortThreads), 0, ctx->stream, keys[cur],              \
                     index_sort && pass == 0 ? (const int *) nullptr                                                   \
                                             : (stride == 2 ? (const int *) keys[cur] + 1 : vals[cur]),                \
                     keys[cur ^ 1], vals[cur ^ 1], n, shift, ntiles, ctx->d_counts.p, d_chunks, chunk_shift, n_dev, stride)
    if (bits == 8) {
      SORT_PASS(8);
    } else if (bits == 9) {
      SORT_PASS(9);
    } else {
      SORT_PASS(10);
    }
#undef SORT_PASS
    cur ^= 1;
  }
  HIPCHK(hipGetLastError());
  *cur_out = cur;
  return 0;
}

int bits_for(unsigned long long kmax) {   // number of key bits that can be non-zero for keys <= kmax
  int key_bits = 1;
  while (key_bits < 32 && (kmax >> key_bits) != 0)
    key_bits++;
  return key_bits;
}

// module_sort keys + sort of (key, index); returns the buffer holding the result
// largest sort key + 1 of the (tiled) cell order; 0 = does not fit 32 bits
int bits_of(unsigned long long v) {   // bits needed for the numbers 0 ... v
  int b = 0;
  while (v >> b)
    b++;
  return b;
}

// tiles of the locality key in Z-order: number of interleaved bit pairs (-1: row-major tile numbers)
int tile_zbits(const mphip_ctx *ctx, int tile) {
  if (tile <= 0 || !ctx->locality_zorder)
    return -1;
  const unsigned long long ntx = (ctx->nx + tile - 1) / tile, nty = (ctx->ny + tile - 1) / tile;
  return std::min(bits_of(ntx - 1), bits_of(nty - 1));
}

unsigned long long sort_key_range(const mphip_ctx *ctx, int tile) {
  unsigned long long kmax = (unsigned long long) ctx->nx * ctx->ny * ctx->npl;
  if (tile > 0) {
    const unsigned long long ntx = (ctx->nx + tile - 1) / tile, nty = (ctx->ny + tile - 1) / tile;
    unsigned long long ntiles = ntx * nty;
    const int m = tile_zbits(ctx, tile);
    if (m >= 0)   // upper bound: every pattern of the interleaved bits under the largest value of the bits on top
      ntiles = ((std::max(ntx - 1, nty - 1) >> m) + 1) << (2 * m);
    kmax = ntiles * ctx->npl * tile * tile;
  }
  return kmax > 0xffffffffULL ? 0 : kmax;
}

// keys of module_sort (and module_timesteps with timestep_t, and module_mixing's box index with box) -> d_keys[0]
int sort_keys(mphip_ctx *ctx, int tile, const double *timestep_t, const BoxArgs *box) {
  if (!sort_key_range(ctx, tile))
    return fail(ctx, "meteo grid too large for the 32-bit sort key");
  const DevMet M = dev_met(ctx);
  const DevAtm a = dev_atm(ctx);
  TimestepArgs ts = { (double) ctx->ctl.direction, ctx->ctl.t_start, ctx->ctl.t_stop, timestep_t ? *timestep_t : 0.0 };
  BoxArgs none;
  memset(&none, 0, sizeof(none));
  const bool lean = ctx->coord_type == 0 && ctx->lut_size > 0 && !ctx->force_generic;
  if (lean)
    hipLaunchKernelGGL(sort_key_kernel<true>, dim3(grid_for(ctx->np)), dim3(256), axes_lds_bytes(ctx), ctx->stream, M, a, tile,
                       tile_zbits(ctx, tile), ctx->d_keys[0].p, (int *) nullptr, ts, timestep_t ? ctx->d_dt.p : nullptr,
                       box ? *box : none);
  else
    hipLaunchKernelGGL(sort_key_kernel<false>, dim3(grid_for(ctx->np)), dim3(256), axes_lds_bytes(ctx), ctx->stream, M, a, tile,
                       tile_zbits(ctx, tile), ctx->d_keys[0].p, (int *) nullptr, ts, timestep_t ? ctx->d_dt.p : nullptr,
                       box ? *box : none);
  HIPCHK(hipGetLastError());
  return 0;
}

int sort_pairs(mphip_ctx *ctx, int tile, int *result_buf, const double *timestep_t) {
  if (sort_keys(ctx, tile, timestep_t, nullptr))
    return 1;
  return radix_passes(ctx, RawPair<uint32_t>(ctx->d_keys).q, RawPair<int>(ctx->d_vals).q, ctx->np,
                      bits_for(sort_key_range(ctx, tile)), result_buf, nullptr, true);
}

// ---- module_sort as a repair of the previous order ---------------------------------------------------------------
// key_prev: the sorted keys of the module_sort whose order the particles are stored in; the new keys are in
// ctx->d_keys[0] (sort_keys).  Leaves the sorted (key, slot) pairs in ctx->d_keys[0] / d_vals[0].
int repair_sort(mphip_ctx *ctx, const uint32_t *key_prev, long long n, int key_bits, int *cur_out) {
  const size_t m = (size_t) n;
  HIPCHK(ctx->rep_sk.reserve(m));
  HIPCHK(ctx->rep_si.reserve(m));
  HIPCHK(ctx->rep_fk.reserve(m));
  HIPCHK(ctx->rep_fv.reserve(m));
  for (int k = 0; k < 2; k++) {
    HIPCHK(ctx->rep_mk[k].reserve(m));
    HIPCHK(ctx->rep_mi[k].reserve(m));
  }
  HIPCHK(ctx->rep_tiles.reserve((m + kRepairTile - 1) / kRepairTile));
  HIPCHK(ctx->rep_nm.reserve(2));
  const int ntiles = (int) ((n + kRepairTile - 1) / kRepairTile);
  const uint32_t *key_new = ctx->d_keys[0].p;
  hipLaunchKernelGGL(repair_count_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, key_new, key_prev, n, ctx->rep_tiles.p);
  hipLaunchKernelGGL(repair_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, ctx->rep_tiles.p, ntiles, n, ctx->rep_nm.p);
  hipLaunchKernelGGL(repair_split_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, key_new, key_prev, n,
                     (const uint32_t *) ctx->rep_tiles.p, ctx->rep_mk[0].p, ctx->rep_mi[0].p, ctx->rep_sk.p, ctx->rep_si.p);
  HIPCHK(hipGetLastError());
  int mc = 0;     // the movers: the stable radix sort over as many pairs as there are (the count stays on the device)
  if (radix_passes(ctx, RawPair<uint32_t>(ctx->rep_mk).q, RawPair<int>(ctx->rep_mi).q, n, key_bits, &mc, ctx->rep_nm.p))
    return 1;
  const int nmerge = (int) ((n + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(repair_merge_kernel, dim3(nmerge), dim3(256), 0, ctx->stream, (const uint32_t *) ctx->rep_sk.p,
                     (const int *) ctx->rep_si.p, (const uint32_t *) ctx->rep_mk[mc].p, (const int *) ctx->rep_mi[mc].p,
                     (const uint32_t *) ctx->rep_nm.p, n, ctx->rep_fk.p, ctx->rep_fv.p);
  HIPCHK(hipGetLastError());
  std::swap(ctx->d_keys[0], ctx->rep_fk);
  std::swap(ctx->d_vals[0], ctx->rep_fv);
  *cur_out = 0;
  return 0;
}

// ---- module_sort ahead of time (mphip_ctx::sort_ahead) -----------------------------------------------------

// the sort buffers of the context <-> the buffers of the sort that runs ahead
void ahead_swap_buffers(mphip_ctx *ctx) {
  for (int k = 0; k < 2; k++) {
    std::swap(ctx->d_keys[k], ctx->ahead_keys[k]);
    std::swap(ctx->d_vals[k], ctx->ahead_vals[k]);
  }
  std::swap(ctx->d_counts, ctx->ahead_counts);
  std::swap(ctx->d_dt, ctx->ahead_dt);
}

// forget a sort that runs ahead (something it depends on is about to change); waits for its kernels, which may
// still be reading the particle arrays
int ahead_drop(mphip_ctx *ctx) {
  if (!ctx->ahead_valid)
    return 0;
  ctx->ahead_valid = false;
  HIPCHK(hipStreamSynchronize(ctx->ahead_stream));
  return 0;
}

// keys, module_timesteps and radix sort of the module_sort call that mphip_run_timestep(t_next) will make, on
// the second stream, behind the kernels queued on the main stream so far
// (box: module_mixing of the current step is still to come -- the key kernel then runs on the main stream and
// leaves the box index of every particle in box->cell on the way, one pass over the particle arrays less)
// stream, events and buffers of the sort ahead
int ahead_ensure(mphip_ctx *ctx) {
  const long long n = ctx->np;
  if (!ctx->ahead_stream) {
    // (with the order repair the sort ahead is little work in few workgroups: at a higher priority they do not queue
    //  behind the thousands of workgroups of the deposition launch)
    int prio_low = 0, prio_high = 0;
    (void) hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    if (ctx->ahead_priority && prio_high != prio_low) {
      HIPCHK(hipStreamCreateWithPriority(&ctx->ahead_stream, hipStreamNonBlocking, prio_high));
    } else
      HIPCHK(hipStreamCreateWithFlags(&ctx->ahead_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ahead_mark, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ahead_done, hipEventDisableTiming));
  }
  for (int k = 0; k < 2; k++) {
    HIPCHK(ctx->ahead_keys[k].reserve((size_t) n));
    HIPCHK(ctx->ahead_vals[k].reserve((size_t) n));
  }
  HIPCHK(ctx->ahead_dt.reserve((size_t) n));
  return 0;
}

// (keys_ready: the launch that moved the particles has written keys, dt and box index already -- EmitKeys)
int ahead_launch(mphip_ctx *ctx, double t_next, const BoxArgs *box = nullptr, bool keys_ready = false) {
  const long long n = ctx->np;
  if (ahead_ensure(ctx))
    return 1;
  // the particles are stored in the order of the last module_sort: its sorted keys (in the buffers of the context, which
  // the sort ahead does not touch) let this one repair that order instead of sorting from scratch
  const uint32_t *key_prev = ctx->sort_repair && ctx->stored_is_sorted && ctx->sorted_buf >= 0 && ctx->sorted_n == n
    ? ctx->d_keys[ctx->sorted_buf].p : nullptr;
  // the sort code runs as it is, on the other stream and the other buffers
  hipStream_t main_stream = ctx->stream;
  ahead_swap_buffers(ctx);
  int cur = 0, rc = 0;
  if (box && !keys_ready)
    rc = sort_keys(ctx, 0, &t_next, box);
  if (!rc && (hipEventRecord(ctx->ahead_mark, main_stream) != hipSuccess
              || hipStreamWaitEvent(ctx->ahead_stream, ctx->ahead_mark, 0) != hipSuccess))
    rc = fail(ctx, "stream hand-over of the sort ahead of time failed");
  ctx->stream = ctx->ahead_stream;
  if (!rc && !box && !keys_ready)
    rc = sort_keys(ctx, 0, &t_next, nullptr);
  if (!rc)
    rc = key_prev ? repair_sort(ctx, key_prev, n, bits_for(sort_key_range(ctx, 0)), &cur)
                  : radix_passes(ctx, RawPair<uint32_t>(ctx->d_keys).q, RawPair<int>(ctx->d_vals).q, n,
                                 bits_for(sort_key_range(ctx, 0)), &cur, nullptr, true);
  ctx->stream = main_stream;
  ahead_swap_buffers(ctx);
  if (rc)
    return 1;
  HIPCHK(hipEventRecord(ctx->ahead_done, ctx->ahead_stream));
  ctx->ahead_valid = true;
  ctx->ahead_t = t_next;
  ctx->ahead_cur = cur;
  ctx->ahead_repaired = key_prev != nullptr;
  return 0;
}

// put every per-particle array back into the external slot order
// The particle arrays of `g` moved by a RANDOM permutation: out[i] = in[index[i]] (gather) or out[index[i]] = in[i]
// (scatter), through one record per particle (perm_pack_kernel / perm_unpack_kernel).  Falls back to the
// array-by-array kernels if the record buffer cannot be had (option perm_records 0 does so always).
int permute_random(mphip_ctx *ctx, const PermArgs &g, const int *index, long long n, bool scatter) {
  const PermGeom pg = perm_geom(n);
  RecordGeom rg;
  rg.n8 = g.n8;
  rg.n4 = g.n4;
  const int words4 = g.n4 + (g.ext_out ? 1 : 0);
  rg.chunks = (g.n8 + 1) / 2 + (words4 + 3) / 4;
  rg.inv = 65536 / rg.chunks + 1;
  for (int p = 0; p < 64 * rg.chunks; p++)
    if ((int) (((unsigned) p * (unsigned) rg.inv) >> 16) != p / rg.chunks)
      return fail(ctx, "internal: record piece index");
  static_assert(sizeof(f32x4u) == 16, "a record piece is 16 bytes");
  const bool records = ctx->perm_records && n >= 65536 && ctx->d_prec.try_reserve((size_t) n * (size_t) rg.chunks);
  if (!records) {
    if (scatter)
      hipLaunchKernelGGL(perm_scatter_kernel, dim3(pg.nblocks), dim3(256), 0, ctx->stream, g, index, n, pg);
    else
      hipLaunchKernelGGL(perm_gather_kernel, dim3(pg.nblocks), dim3(256), 0, ctx->stream, g, index, n, pg);
    HIPCHK(hipGetLastError());
    return 0;
  }
  f32x4u *rec = ctx->d_prec.p;
  const size_t lds = (size_t) kRecordWaves * 64 * (size_t) rg.chunks * 16;
  hipLaunchKernelGGL(perm_pack_kernel, dim3(pg.nblocks), dim3(64 * kRecordWaves), lds, ctx->stream, g, rg,
                     scatter ? index : (const int *) nullptr, rec, n, pg);
  hipLaunchKernelGGL(perm_unpack_kernel, dim3(pg.nblocks), dim3(64 * kRecordWaves), lds, ctx->stream, g, rg,
                     scatter ? (const int *) nullptr : index, (const f32x4u *) rec, n, pg);
  HIPCHK(hipGetLastError());
  return 0;
}

int restore_external_order(mphip_ctx *ctx) {
  if (ctx->ext_identity || ctx->np == 0) {
    ctx->ext_identity = true;
    return 0;
  }
  if (ahead_drop(ctx))
    return 1;
  PermArgs g = perm_args(ctx, true);
  if (permute_random(ctx, g, ctx->d_ext.p, ctx->np, true))
    return 1;
  perm_swap(ctx, true);
  ctx->stored_is_sorted = false;
  ctx->ext_identity = true;
  ctx->steps_since_resort = 1 << 30;
  return 0;
}

// internal locality order: store the particles sorted by the grid cell their
// interpolation stencil starts in.  Nothing observable changes: random numbers
// follow the external slot (d_ext) and downloads restore the external order.
// First half: keys and radix sort; *cur = the buffer pair that holds the sorted (key, slot) pairs.
int locality_sort_keys(mphip_ctx *ctx, int *cur) {
  if (ahead_drop(ctx) || ensure_packed(ctx))
    return 1;
  // measured (tools/gpu_ablate.py tiles): 4 x 4 columns for the pressure-level kernels, 8 x 8 for the model-level ones
  const int tile = ctx->locality_tile > 0 ? ctx->locality_tile : (ctx->have_ctl && ml_winds(ctx->ctl) ? 8 : 4);
  return sort_pairs(ctx, tile, cur, nullptr);
}

// Second half: every per-particle array moves by the sorted slots.  fold: no pass of its own -- the caller's next
// launch, a lean multi-step one, reads its per-launch loads through the permutation (ctx->fold_perm, DevAtm::perm_all;
// a re-sort only: `ext` composes with the one in place) and the caller clears the hand-over behind that launch.
int locality_sort_apply(mphip_ctx *ctx, int cur, bool fold) {
  PermArgs g = perm_args(ctx, true);
  g.ext_in = ctx->ext_identity ? nullptr : ctx->d_ext.p;
  g.ext_out = ctx->d_ext_alt.p;
  if (fold) {
    ctx->fold_perm = ctx->d_vals[cur].p;
  } else if (ctx->ext_identity) {   // out of the caller's order: a random permutation
    if (permute_random(ctx, g, ctx->d_vals[cur].p, ctx->np, false))
      return 1;
  } else {                   // a re-sort: most particles stay where they are, the gathers hit the caches
    const PermGeom pg = perm_geom(ctx->np);
    hipLaunchKernelGGL(perm_gather_kernel, dim3(pg.nblocks), dim3(256), 0, ctx->stream, g, ctx->d_vals[cur].p, ctx->np, pg);
    HIPCHK(hipGetLastError());
  }
  perm_swap(ctx, true);
  std::swap(ctx->d_ext, ctx->d_ext_alt);
  ctx->stored_is_sorted = false;
  ctx->ext_identity = false;
  ctx->steps_since_resort = 0;
  return 0;
}

int locality_sort(mphip_ctx *ctx) {
  if (ctx->np == 0)
    return 0;
  int cur = 0;
  return locality_sort_keys(ctx, &cur) || locality_sort_apply(ctx, cur, false);
}

// module_sort, mptrac.c:5887-5957: observable re-ordering of atm (time, p, lon,
// lat, q[*]); cache->uvwp and cache->dt stay with their slots as in the
// reference.
int do_sort(mphip_ctx *ctx, const double *timestep_t = nullptr) {
  const long long n = ctx->np;
  if (n == 0)
    return 0;
  int cur = 0;
  if (timestep_t && ctx->ahead_valid && ctx->ahead_t == *timestep_t && ctx->ext_identity) {
    // keys, dt and the sorted permutation were computed beside the previous time step: take them over
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ahead_done, 0));
    ahead_swap_buffers(ctx);
    ctx->ahead_valid = false;
    cur = ctx->ahead_cur;
    (ctx->ahead_repaired ? ctx->sorts_repaired : ctx->sorts_scratch)++;
  } else {
    const bool internal = !ctx->ext_identity;   // stored in the internal locality order: undone first
    if (ahead_drop(ctx) || ensure_packed(ctx) || restore_external_order(ctx))
      return 1;
    if (sort_pairs(ctx, 0, &cur, timestep_t))   // with timestep_t: module_timesteps in the key kernel
      return 1;
    ctx->sorts_scratch++;
    ctx->sorts_undone += internal;
  }
  ctx->sorted_buf = cur;
  ctx->stored_is_sorted = true;      // (once the gather below -- or the step launch that carries it -- has run)
  ctx->sorted_n = n;
  const PermGeom pg = perm_geom(n);
  if (timestep_t && ctx->fuse_sort) {
    // inside mphip_run_timestep the step launch that follows reads time, p, lon, lat through the
    // permutation and writes them in the new order (DevAtm::perm); only the quantity arrays move here
    PermArgs g;
    memset(&g, 0, sizeof(g));
    g.n8 = ctx->nq;
    for (int k = 0; k < ctx->nq; k++) {
      g.in8[k] = ctx->d_arr[4 + k].p;
      g.out8[k] = ctx->d_alt[4 + k].p;
    }
    // ... or not even those: option fuse_sort_quantities (default) lets the step launch move them as well
    ctx->fused_quantities = ctx->fuse_quantities;
    if (ctx->nq > 0 && !ctx->fused_quantities) {
      hipLaunchKernelGGL(perm_gather_kernel, dim3(pg.nblocks), dim3(256), 0, ctx->stream, g, ctx->d_vals[cur].p, n, pg);
      HIPCHK(hipGetLastError());
    }
    for (int k = 0; k < 4 + ctx->nq; k++)
      std::swap(ctx->d_arr[k], ctx->d_alt[k]);   // d_alt[0..3] now hold the pre-sort time, p, lon, lat
    ctx->fused_perm = ctx->d_vals[cur].p;
  } else {
    PermArgs g = perm_args(ctx, false);
    hipLaunchKernelGGL(perm_gather_kernel, dim3(pg.nblocks), dim3(256), 0, ctx->stream, g, ctx->d_vals[cur].p, n, pg);
    HIPCHK(hipGetLastError());
    perm_swap(ctx, false);
  }
  ctx->steps_since_resort = 0;   // the observable order is a locality order already
  return 0;
}

// grow-only with a hard failure, for the `||` chains of this file (a statement of its own: HIPCHK(buf.reserve(n)))
template <typename B>
int reserve(mphip_ctx *ctx, B &buf, size_t n) {
  HIPCHK(buf.reserve(n));
  return 0;
}

// ---- RCCL (loaded on first use: single-GPU callers need no librccl) ------------
// Only the handful of entry points the gridded reductions need; types restated from rccl.h (stable NCCL ABI).
struct Rccl {
  typedef struct { char internal[128]; } UniqueId;
  int (*GetUniqueId)(UniqueId *) = nullptr;
  int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  int (*CommUserRank)(void *, int *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  bool ok = false;
  std::string why;
};
constexpr int kNcclInt32 = 2, kNcclFloat64 = 8, kNcclSum = 0;

Rccl &rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    void *h = nullptr;
    for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" })
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)))
        break;
    if (!h) {
      r.why = std::string("cannot load librccl.so: ") + dlerror();
      return;
    }
    auto sym = [&](const char *n) {
      void *p = dlsym(h, n);
      if (!p)
        r.why = std::string("librccl.so lacks ") + n;
      return p;
    };
    r.GetUniqueId = (decltype(r.GetUniqueId)) sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank)) sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy)) sym("ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce)) sym("ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart)) sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd)) sym("ncclGroupEnd");
    r.CommCount = (decltype(r.CommCount)) sym("ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank)) sym("ncclCommUserRank");
    r.GetErrorString = (decltype(r.GetErrorString)) sym("ncclGetErrorString");
    r.ok = r.why.empty();
  });
  return r;
}

// RCCL writes a version banner to stdout when it initialises; callers of this library own stdout (bench.py
// prints exactly one JSON line there), so the banner goes to stderr instead
struct StdoutToStderr {
  int saved = -1;
  StdoutToStderr() {
    fflush(stdout);
    saved = dup(1);
    if (saved >= 0)
      dup2(2, 1);
  }
  ~StdoutToStderr() {
    fflush(stdout);
    if (saved >= 0) {
      dup2(saved, 1);
      close(saved);
    }
  }
};

#define RCCLCHK(call)                                                                        \
  do {                                                                                       \
    const int e_ = (call);                                                                   \
    if (e_ != 0)                                                                             \
      return fail(ctx, std::string(#call) + ": " + rccl().GetErrorString(e_));               \
  } while (0)

// Sum over the ranks, in place: `count` doubles at dbuf and (optionally) `icount` 32-bit integers at ibuf.
// With a communicator (mphip_comm_init) both go to RCCL as one group on the context's stream and the host does
// not wait; with an all-reduce hook (tests, staged host collectives) the stream is drained and the integers
// travel as doubles in `scratch` (icount doubles).
int run_allreduce(mphip_ctx *ctx, double *dbuf, size_t count, int *ibuf = nullptr, size_t icount = 0,
                  double *scratch = nullptr) {
  if (ctx->comm) {
    Rccl &R = rccl();
    RCCLCHK(R.GroupStart());
    if (count)
      RCCLCHK(R.AllReduce(dbuf, dbuf, count, kNcclFloat64, kNcclSum, ctx->comm, ctx->stream));
    if (icount)
      RCCLCHK(R.AllReduce(ibuf, ibuf, icount, kNcclInt32, kNcclSum, ctx->comm, ctx->stream));
    RCCLCHK(R.GroupEnd());
    return 0;
  }
  if (!ctx->allreduce)
    return 0;
  if (icount) {
    hipLaunchKernelGGL(int_to_double_kernel, dim3(grid_for((long long) icount)), dim3(256), 0, ctx->stream, ibuf, scratch,
                       icount);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (count && ctx->allreduce(dbuf, count, ctx->allreduce_user))
    return fail(ctx, "all-reduce hook reported an error");
  if (icount) {
    if (ctx->allreduce(scratch, icount, ctx->allreduce_user))
      return fail(ctx, "all-reduce hook reported an error");
    hipLaunchKernelGGL(double_to_int_kernel, dim3(grid_for((long long) icount)), dim3(256), 0, ctx->stream, scratch, ibuf,
                       icount);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// module_mixing, mptrac.c:5169-5347
// launch geometry of the LDS-table accumulation kernels: table entries (power of two) that fit in
// 64 kB of LDS for nv doubles per entry, and contiguous runs of the stored order per block
struct AccumGeom {
  int T, nblocks;
  long long per_block;
  size_t lds;
};

AccumGeom accum_geom(const mphip_ctx *ctx, int nv) {
  AccumGeom g;
  g.T = 2048;
  while (g.T > 64 && (size_t) g.T * (8 * (size_t) nv + 4) > 64 * 1024)
    g.T >>= 1;
  g.lds = (size_t) g.T * (8 * (size_t) nv + 4);
  long long per_block = (ctx->np + 4095) / 4096;
  per_block = std::max<long long>(256, (per_block + 255) / 256 * 256);
  g.per_block = per_block;
  g.nblocks = (int) std::max<long long>(1, (ctx->np + per_block - 1) / per_block);
  return g;
}

// Sums of VALS per cell in the reference's serial order (steps 1-4 of "Cell sums" in mphip_kernels.hpp).
// ctx->d_cell holds the cell of every stored particle; writes sums[v * ntot + cell] (nv values) and the counts
// as integers and / or doubles (either may be NULL).
// `every_cell`: cells of groups without particles must read zero afterwards (an all-reduce or the host looks at
// all of them); module_mixing on a single rank only ever reads the cells its particles are in, which the
// group kernel has written, and skips the clearing passes
// (box: the cells are write_grid's box indices and have not been computed yet -- the crowded-cell path does that on
//  its way; the other path calls box_index_kernel first)
template <class VALS>
int ordered_cell_sums(mphip_ctx *ctx, const VALS &vals, int nv, int column, size_t ntot, double *sums, int *cnt,
                      double *cnt_as_double, bool every_cell = true, const GridBoxArgs *box = nullptr) {
  const long long n = ctx->np;
  // cells per group: whole vertical columns of the grid, as many as fit the table in LDS while there are
  // still >= 2^14 groups to spread over the waves
  int G = kGroupMax;
  if (column >= 1 && column <= kGroupMax) {
    const size_t ncol = std::max<size_t>(1, std::min<size_t>(kGroupMax / column, ntot / column / 16384));
    G = column * (int) ncol;
  }
  const size_t ngroups = (ntot + G - 1) / G;
  if (ntot >= 0x7fffffffULL)
    return fail(ctx, "too many grid cells for 32-bit cell indices");
  // crowded cells (a 2-D output grid, a dense plume on a coarse grid): sort the whole particle list by cell and
  // give every (cell, value) chain a lane -- "crowded cells" in mphip_kernels.hpp
  const bool chains = ctx->sum_path == 2 || (ctx->sum_path == 0 && (double) n >= 16.0 * (double) ntot);
  if (chains && n > 0) {
    const size_t words32 = 4 * (size_t) n;
    HIPCHK(ctx->d_lists.reserve((words32 + 1) / 2));
    uint32_t *base = (uint32_t *) ctx->d_lists.p;
    uint32_t *keys[2] = { base, base + 2 * n };
    int *slots[2] = { (int *) (base + n), (int *) (base + 3 * n) };
    // (cell, slot) pairs in external order, interleaved in the first half of the buffer; the first pass of the
    // sort reads them from there and writes the second half
    GridBoxArgs gb;
    memset(&gb, 0, sizeof(gb));
    if (box)
      gb = *box;
    hipLaunchKernelGGL(cell_slot_pairs_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->stream, ctx->d_cell.p,
                       ctx->ext_identity ? (const int *) nullptr : ctx->d_ext.p, n, (uint32_t) ntot, (uint2 *) base, gb,
                       box ? 1 : 0);
    int cur = 0;
    if (radix_passes(ctx, keys, slots, n, bits_for(ntot), &cur, nullptr, false, true))
      return 1;
    const int width = nv < 1 ? 1 : nv < 64 ? nv : 64;   // nv == 0: counts only (gridded output without quantities)
    const long long waves = ((long long) ntot + 64 / width - 1) / (64 / width);
    // (measured on C3's output, 1e7 particles on 360 x 180 cells: 1.10 ms per output with every wave resident,
    // 1.21 / 1.36 / 1.86 ms with 512 / 256 / 64 workgroups -- the gathers are bound by the 128-byte lines they
    // pull for 8 bytes each, 3.1 GB per output, and fewer waves in flight do not make the lines live longer)
    int chain_blocks = ctx->chain_blocks > 0 ? ctx->chain_blocks : 8192;
    // (a multiple of 8 workgroups: the kernel maps them to contiguous runs of cells per XCD)
    chain_blocks = std::max(8, std::min(chain_blocks, (grid_for(waves * 64) + 7) & ~7) & ~7);
    // every cell finds its range of the sorted list itself (a pass over the list and a clearing pass less)
    hipLaunchKernelGGL(cell_sum_chains_kernel<VALS>, dim3(chain_blocks), dim3(256), 0, ctx->stream, vals,
                       slots[cur], keys[cur], n, ntot, sums, cnt, cnt_as_double);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (box && n > 0)   // the other path works on ctx->d_cell
    hipLaunchKernelGGL(box_index_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->stream, dev_atm(ctx), box->G, box->t0,
                       box->t1, ctx->d_cell.p, (const double *) nullptr, 0);
  if (every_cell) {
    HIPCHK(hipMemsetAsync(sums, 0, (size_t) nv * ntot * sizeof(double), ctx->stream));
    if (cnt)
      HIPCHK(hipMemsetAsync(cnt, 0, ntot * sizeof(int), ctx->stream));
    if (cnt_as_double)
      HIPCHK(hipMemsetAsync(cnt_as_double, 0, ntot * sizeof(double), ctx->stream));
  }
  if (n == 0)
    return 0;
  // one allocation, 32-bit words: [sequence cell | sequence slot | keys 0 | ids 0 | keys 1 | ids 1 | run starts
  // (n + 1) | runs per tile (ntiles + 1) | overflow flag]
  const int ntiles = (int) ((n + kRunTile - 1) / kRunTile);
  const size_t words32 = 7 * (size_t) n + 1 + (size_t) ntiles + 1 + 1;
  HIPCHK(ctx->d_lists.reserve((words32 + 1) / 2));
  uint32_t *base = (uint32_t *) ctx->d_lists.p;
  int *seq_cell = (int *) base, *seq_slot = (int *) (base + n);
  uint32_t *keys[2] = { base + 2 * n, base + 4 * n };
  int *ids[2] = { (int *) (base + 3 * n), (int *) (base + 5 * n) };
  uint32_t *run_start = base + 6 * n, *tile_runs = base + 7 * n + 1;
  int *overflow = (int *) (tile_runs + ntiles + 1);
  const uint32_t *nruns_dev = tile_runs + ntiles;   // stays on the device: the launches cover the upper bound n
  const int nblocks = (int) std::min<long long>((n + 255) / 256, 16384);
  const int key_bits = bits_for(ngroups);
  // runs of `seq`, sorted by group -> keys[cur], ids[cur] (kernels do nothing while *gate == 0)
  auto sorted_runs = [&](const int *seq, const int *gate, int *cur) -> int {
    hipLaunchKernelGGL(run_heads_count_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, seq, n, G, tile_runs, gate);
    hipLaunchKernelGGL(run_offsets_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, tile_runs, ntiles, gate);
    hipLaunchKernelGGL(run_compact_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, seq, n, G, tile_runs, ntiles,
                       (uint32_t) ngroups, keys[0], (int *) nullptr, run_start, gate);
    return radix_passes(ctx, keys, ids, n, key_bits, cur, nruns_dev, true);
  };
#define GROUPS(B, BYINDEX, SEQ, SLOT)                                                                                  \
  hipLaunchKernelGGL((cell_sum_groups_kernel<VALS, B, BYINDEX>), dim3(nblocks), dim3(256), 0, ctx->stream, vals,       \
                     keys[cur], ids[cur], nruns_dev, (uint32_t) ngroups, run_start, SEQ, SLOT, ctx->d_ext.p, overflow, G, \
                     ntot, sums, cnt, cnt_as_double)
#define GROUPS_BY_WIDTH(BYINDEX, SEQ, SLOT)                                                                            \
  if (nv <= 1) {   /* values per pass: as many as there are, up to four */                                             \
    GROUPS(1, BYINDEX, SEQ, SLOT);                                                                                     \
  } else if (nv == 2) {                                                                                                \
    GROUPS(2, BYINDEX, SEQ, SLOT);                                                                                     \
  } else if (nv == 3) {                                                                                                \
    GROUPS(3, BYINDEX, SEQ, SLOT);                                                                                     \
  } else {                                                                                                             \
    GROUPS(4, BYINDEX, SEQ, SLOT);                                                                                     \
  }
  int cur = 0;
  if (ctx->ext_identity) {
    // the stored order is the external order (after module_sort): stream the groups as they come
    if (sorted_runs(ctx->d_cell.p, nullptr, &cur))
      return 1;
    GROUPS_BY_WIDTH(false, ctx->d_cell.p, (const int *) nullptr)
  } else {
    // internal locality order: the runs of the STORED order are long; every wave puts its group into index
    // order in LDS.  A group that does not fit there raises the flag ...  (With hundreds of particles per
    // group -- a 2-D output grid -- the sort in LDS costs more than the general pass: 2.3 against 1.5 ms for
    // 1e7 particles on 360 x 180 cells; that case goes to the general pass directly.)
    const bool in_lds = (double) n / (double) ngroups <= 256.0;
    HIPCHK(hipMemsetAsync(overflow, in_lds ? 0 : 1, sizeof(int), ctx->stream));
    if (in_lds) {
      if (sorted_runs(ctx->d_cell.p, nullptr, &cur))
        return 1;
      GROUPS_BY_WIDTH(true, ctx->d_cell.p, (const int *) nullptr)
    }
    // ... and the general pass runs: the whole sequence laid out in external order (one run per particle, the
    // permutation is random in the index), same kernels.  Without the flag its launches return at once.
    hipLaunchKernelGGL(cell_pairs_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->stream, ctx->d_cell.p, ctx->d_ext.p, n,
                       seq_cell, seq_slot, overflow);
    if (sorted_runs(seq_cell, overflow, &cur))
      return 1;
    GROUPS_BY_WIDTH(false, seq_cell, seq_slot)
  }
#undef GROUPS_BY_WIDTH
#undef GROUPS
  HIPCHK(hipGetLastError());
  return 0;
}

// module_mixing, mptrac.c:5169-5347:
//   mixing_plan   what is mixed, the grid, the buffers
//   mixing_cells  the box of every particle
//   mixing_sums   sums and counts per box, all-reduce over the ranks
//   mixing_relax  every particle towards the mean of its box
struct MixGrid {
  BoxGrid grid;
  double t0, t1;
  const double *ens;
  int ngrid;
};

struct MixPlan {
  MixGrid box;      // the grid and the time window
  MixSet mq;        // what is mixed
  size_t ntot;      // boxes (times ensemble members)
};

// false in *active: nothing to mix
int mixing_plan(mphip_ctx *ctx, double t, MixPlan *P, bool *active) {
  const mphip_ctl_t &c = ctx->ctl;
  *active = false;
  if (!ctx->have_clim)
    return fail(ctx, "climatological tropopause data were not uploaded");
  const int ngrid = c.mixing_nx * c.mixing_ny * c.mixing_nz;
  const int nens = c.nens > 0 ? c.nens : 1;
  const size_t ntot = (size_t) ngrid * nens;
  const DevAtm a = dev_atm(ctx);
  memset(P, 0, sizeof(*P));
  // the mixed quantities (hot-path subset of mptrac.c:5223-5230), all in one pass
  MixSet &mq = P->mq;
  for (int iq : { c.qnt_m, c.qnt_vmr, c.qnt_tracer[MPHIP_TR_CCL4], c.qnt_tracer[MPHIP_TR_CCL3F], c.qnt_tracer[MPHIP_TR_CCL2F2],
                  c.qnt_tracer[MPHIP_TR_N2O], c.qnt_tracer[MPHIP_TR_SF6], c.qnt_aoa })
    if (iq >= 0)
      mq.q[mq.n++] = a.q[iq];
  for (int iq : ctx->radio.q)   // ... and the activities registered with mphip_set_radio_decay
    if (iq >= 0)
      mq.q[mq.n++] = a.q[iq];
  if (mq.n == 0)
    return 0;
  // [sums of quantity 0 | 1 | 2 | scratch for a doubles-only all-reduce hook]
  const bool hook = !ctx->comm && ctx->allreduce;
  if (reserve(ctx, ctx->d_sums, ((size_t) mq.n + (hook ? 1 : 0)) * ntot) || reserve(ctx, ctx->d_cnt, ntot))
    return 1;
  P->ntot = ntot;
  P->box.grid = BoxGrid{ c.mixing_lon0, c.mixing_lon1, c.mixing_lat0, c.mixing_lat1, c.mixing_z0, c.mixing_z1,
                          c.mixing_nx, c.mixing_ny, c.mixing_nz };
  P->box.t0 = t - 0.5 * c.dt_mod;
  P->box.t1 = t + 0.5 * c.dt_mod;
  P->box.ens = (c.nens > 0 && c.qnt_ens >= 0) ? a.q[c.qnt_ens] : nullptr;
  P->box.ngrid = ngrid;
  *active = true;
  return 0;
}

int mixing_cells(mphip_ctx *ctx, const MixPlan &P) {
  if (ctx->np == 0)
    return 0;
  const MixGrid &h = P.box;
  hipLaunchKernelGGL(box_index_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, dev_atm(ctx), h.grid, h.t0, h.t1,
                     ctx->d_cell.p, h.ens, h.ngrid);
  HIPCHK(hipGetLastError());
  return 0;
}

// The exchange of a mixing step restricted to the band of levels that holds particles on any rank (SURVEY 8e (2):
// 5.83e6 boxes x 12 B = 70 MB per mixed quantity and step for the default grid; the particles of BASELINE configs[4]
// occupy 31 of its 90 levels).  A small all-reduce of the per-level occupancy first (nz doubles), its result read by
// the host -- the one synchronisation of the step path, taken only by runs of several ranks --, then pack, all-reduce
// of the band, unpack.  The boxes outside the band hold no particle on any rank: nothing to add there, and every box
// inside adds the same partial sums in the same order as the exchange of the whole grid (identical bits:
// test_mixing_exchange_of_the_occupied_levels_equals_the_whole_grid).  Falls back to the whole grid when the band
// covers four fifths of it.
int exchange_occupied_levels(mphip_ctx *ctx, int nq, size_t ntot, int nz) {
  const size_t ncol = ntot / (size_t) nz;
  HIPCHK(ctx->d_occ.reserve(256));   // (both or neither: a failure of either returns before any use)
  HIPCHK(ctx->h_occ.reserve(256));
  HIPCHK(hipMemsetAsync(ctx->d_occ.p, 0, (size_t) nz * sizeof(double), ctx->stream));
  hipLaunchKernelGGL(level_occupancy_kernel, dim3(std::min<size_t>(1024, (ntot + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const int *) ctx->d_cnt.p, ntot, nz, ctx->d_occ.p);
  HIPCHK(hipGetLastError());
  if (run_allreduce(ctx, ctx->d_occ.p, (size_t) nz))
    return 1;
  HIPCHK(hipMemcpyAsync(ctx->h_occ.p, ctx->d_occ.p, (size_t) nz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int lo = nz, hi = -1;
  for (int l = 0; l < nz; l++)
    if (ctx->h_occ.p[l] > 0) {
      lo = std::min(lo, l);
      hi = std::max(hi, l);
    }
  ctx->mix_band_lo = lo;
  ctx->mix_band_hi = hi;
  if (hi < lo)        // no particle in any box on any rank: nothing to exchange
    return 0;
  const int nl = hi - lo + 1;
  if (5 * nl >= 4 * nz)
    return run_allreduce(ctx, ctx->d_sums.p, (size_t) nq * ntot, ctx->d_cnt.p, ntot, ctx->d_sums.p + (size_t) nq * ntot);
  const size_t per = ncol * (size_t) nl;
  // dense buffers: [sums of the quantities | scratch for a doubles-only hook] and the counts
  HIPCHK(ctx->d_band.reserve(((size_t) nq + 1) * per));
  HIPCHK(ctx->d_band_cnt.reserve(per));
  const int blocks = (int) std::min<size_t>(8192, ((size_t) nq * per + 255) / 256);
  hipLaunchKernelGGL(pack_levels_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream, (const double *) ctx->d_sums.p,
                     ctx->d_band.p, ncol, nz, lo, nl, nq, false, (double *) nullptr);
  hipLaunchKernelGGL(pack_levels_kernel<int>, dim3(blocks), dim3(256), 0, ctx->stream, (const int *) ctx->d_cnt.p,
                     ctx->d_band_cnt.p, ncol, nz, lo, nl, 1, false, (int *) nullptr);
  HIPCHK(hipGetLastError());
  if (run_allreduce(ctx, ctx->d_band.p, (size_t) nq * per, ctx->d_band_cnt.p, per, ctx->d_band.p + (size_t) nq * per))
    return 1;
  hipLaunchKernelGGL(pack_levels_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream, (const double *) nullptr,
                     ctx->d_band.p, ncol, nz, lo, nl, nq, true, ctx->d_sums.p);
  hipLaunchKernelGGL(pack_levels_kernel<int>, dim3(blocks), dim3(256), 0, ctx->stream, (const int *) nullptr,
                     ctx->d_band_cnt.p, ncol, nz, lo, nl, 1, true, ctx->d_cnt.p);
  HIPCHK(hipGetLastError());
  return 0;
}

// (every_cell: every cell must read its sums and count afterwards, also the empty ones -- module_chem_grid's table)
int mixing_sums(mphip_ctx *ctx, const MixPlan &P, bool every_cell = false) {
  const MixSet &mq = P.mq;
  const size_t ntot = P.ntot;
  if (ctx->deterministic_sums != 0) {
    MixVals vals = { mq };
    const bool exchanged = ctx->comm != nullptr || ctx->allreduce != nullptr;
    if (ordered_cell_sums(ctx, vals, mq.n, P.box.grid.nz, ntot, ctx->d_sums.p, ctx->d_cnt.p, (double *) nullptr,
                          exchanged || every_cell))
      return 1;
  } else {
    HIPCHK(hipMemsetAsync(ctx->d_sums.p, 0, (size_t) mq.n * ntot * sizeof(double), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_cnt.p, 0, ntot * sizeof(int), ctx->stream));
    if (ctx->np) {
      const AccumGeom g = accum_geom(ctx, mq.n + 1);
      hipLaunchKernelGGL(mix_accumulate_kernel, dim3(g.nblocks), dim3(256), g.lds, ctx->stream, dev_atm(ctx), ctx->d_cell.p,
                         mq, ntot, ctx->d_sums.p, ctx->d_cnt.p, g.T, g.per_block);
      HIPCHK(hipGetLastError());
    }
  }
  // one exchange per mixing step: the sums of every mixed quantity and the cell counts
  const bool exchange = ctx->comm != nullptr || ctx->allreduce != nullptr;
  const int nz = P.box.grid.nz;
  if (exchange && ctx->mix_exchange_levels && nz >= 8 && nz <= 256 && ntot >= ((size_t) 1 << 18))
    return exchange_occupied_levels(ctx, mq.n, ntot, nz);
  return run_allreduce(ctx, ctx->d_sums.p, (size_t) mq.n * ntot, ctx->d_cnt.p, ntot, ctx->d_sums.p + (size_t) mq.n * ntot);
}

int mixing_relax(mphip_ctx *ctx, const MixPlan &P) {
  if (ctx->np == 0)
    return 0;
  hipLaunchKernelGGL(mix_relax_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, ctx->ctl, ctx->d_clim.p,
                     dev_atm(ctx), ctx->d_cell.p, P.mq, P.ntot, ctx->d_sums.p, ctx->d_cnt.p);
  HIPCHK(hipGetLastError());
  return 0;
}

// (cells_ready: the box indices are in d_cell already, left there by the key kernel of a sort ahead of time)
int do_mixing(mphip_ctx *ctx, double t, bool cells_ready = false) {
  MixPlan P;
  bool active;
  if (mixing_plan(ctx, t, &P, &active))
    return 1;
  if (!active)
    return 0;
  return (!cells_ready && mixing_cells(ctx, P)) || mixing_sums(ctx, P) || mixing_relax(ctx, P);
}

// module_chem_grid: the mass per cell of the chemistry grid turned into a volume mixing ratio, written into quantity Cx
// of every particle in the cell.  Reuses module_mixing's pieces: the box index (box_cell: time window
// [t - DT_MOD / 2, t + DT_MOD / 2], inside the grid, ensemble offset), the cell sums of one value -- q[m] -- in the
// serial order (atomics with deterministic_sums 0), the all-reduce of sums and counts over the ranks.  Then a table of
// Cx over the occupied cells (the cell-centre temperature once per cell) and a gather per particle.
bool chem_on(const mphip_ctl_t &c) {
  return c.oh_chem_reaction != 0 || c.h2o2_chem_reaction != 0;
}

bool chemgrid_valid(const mphip_ctl_t &c) {
  return c.chemgrid_nx >= 1 && c.chemgrid_ny >= 1 && c.chemgrid_nz >= 1 && c.chemgrid_lon0 < c.chemgrid_lon1
    && c.chemgrid_lat0 < c.chemgrid_lat1 && c.chemgrid_z0 < c.chemgrid_z1;
}

int do_chem_grid(mphip_ctx *ctx, double t) {
  const mphip_ctl_t &c = ctx->ctl;
  if (c.qnt_m < 0 || c.qnt_Cx < 0)
    return 0;
  if (c.molmass <= 0)
    return fail(ctx, "module_chem_grid: Molar mass is not defined!");
  if (!chemgrid_valid(c) || !ctx->chemgrid_ok)
    return fail(ctx, "module_chem_grid: invalid chemistry grid (CHEMGRID_NX / NY / NZ >= 1 and non-empty "
                     "CHEMGRID_LON0 < LON1, LAT0 < LAT1, Z0 < Z1)");
  if (ctx->np > 0) {
    if (ensure_packed(ctx))
      return 1;
    if (!both_have(ctx, 1u << MPHIP_T))
      return fail(ctx, "module_chem_grid: meteo field t was not uploaded");
  }
  const long long ngrid = (long long) c.chemgrid_nx * c.chemgrid_ny * c.chemgrid_nz;
  const int nens = c.nens > 0 ? c.nens : 1;
  if (ngrid * nens >= 0x7fffffffLL)
    return fail(ctx, "module_chem_grid: too many grid cells for 32-bit cell indices");
  const size_t ntot = (size_t) ngrid * nens;
  const DevAtm a = dev_atm(ctx);
  MixPlan P;
  memset(&P, 0, sizeof(P));
  P.mq.q[0] = a.q[c.qnt_m];
  P.mq.n = 1;
  P.ntot = ntot;
  P.box.grid = BoxGrid{ c.chemgrid_lon0, c.chemgrid_lon1, c.chemgrid_lat0, c.chemgrid_lat1, c.chemgrid_z0, c.chemgrid_z1,
                        c.chemgrid_nx, c.chemgrid_ny, c.chemgrid_nz };
  P.box.t0 = t - 0.5 * c.dt_mod;
  P.box.t1 = t + 0.5 * c.dt_mod;
  P.box.ens = (c.nens > 0 && c.qnt_ens >= 0) ? a.q[c.qnt_ens] : nullptr;
  P.box.ngrid = (int) ngrid;
  const bool hook = !ctx->comm && ctx->allreduce;
  if (reserve(ctx, ctx->d_sums, (1 + (hook ? 1 : 0)) * ntot) || reserve(ctx, ctx->d_cnt, ntot))
    return 1;
  if (mixing_cells(ctx, P) || mixing_sums(ctx, P, true))
    return 1;
  ChemGridArgs C;
  C.press = ctx->d_chemgrid.p;
  C.area = C.press + c.chemgrid_nz;
  C.lon = C.area + c.chemgrid_ny;
  C.lat = C.lon + c.chemgrid_nx;
  C.dz = (c.chemgrid_z1 - c.chemgrid_z0) / c.chemgrid_nz;
  C.molmass = c.molmass;
  C.tt = t;
  C.nx = c.chemgrid_nx;
  C.ny = c.chemgrid_ny;
  C.nz = c.chemgrid_nz;
  C.ngrid = (int) ngrid;
  C.ntot = (long long) ntot;
  C.val = ctx->d_sums.p;
  C.cnt = ctx->d_cnt.p;
  if (ctx->np == 0)   // (a rank without particles takes part in the all-reduce only)
    return 0;
  hipLaunchKernelGGL(chem_grid_table_kernel, dim3(grid_for((long long) ntot)), dim3(256), axes_lds_bytes(ctx), ctx->stream,
                     dev_met(ctx), C);
  hipLaunchKernelGGL(chem_grid_gather_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, a,
                     (const int *) ctx->d_cell.p, (const double *) ctx->d_sums.p, c.qnt_Cx);
  HIPCHK(hipGetLastError());
  return 0;
}

// module_radio_decay: an activity is registered; the bit of the step kernel's tail when the module is on (nothing to do
// without an activity: no bit)
bool radio_any(const mphip_ctx *ctx) {
  for (int iq : ctx->radio.q)
    if (iq >= 0)
      return true;
  return false;
}

unsigned radio_step_bit(const mphip_ctx *ctx) {
  return ctx->radio_on && radio_any(ctx) ? kRadioDecay : 0u;
}

// what mphip_set_radio_decay refuses for the activities q[] under the control parameters c ("" = nothing)
std::string radio_conflict(const mphip_ctl_t &c, const int *q) {
  static const char *const names[MPHIP_NRADIO] = { "Arn222", "Apb210", "Abe7", "Acs137", "Ai131", "Axe133" };
  const struct {
    int iq;
    const char *what;
  } taken[] = { { c.qnt_m, "m" }, { c.qnt_vmr, "vmr" }, { c.qnt_loss_rate, "loss_rate" },
                { c.qnt_mloss_decay, "mloss_decay" }, { c.qnt_mloss_wet, "mloss_wet" }, { c.qnt_mloss_dry, "mloss_dry" },
                { c.qnt_mloss_oh, "mloss_oh" }, { c.qnt_mloss_h2o2, "mloss_h2o2" }, { c.qnt_aoa, "aoa" },
                { c.qnt_tracer[MPHIP_TR_CCL4], "Cccl4" }, { c.qnt_tracer[MPHIP_TR_CCL3F], "Cccl3f" },
                { c.qnt_tracer[MPHIP_TR_CCL2F2], "Cccl2f2" }, { c.qnt_tracer[MPHIP_TR_N2O], "Cn2o" },
                { c.qnt_tracer[MPHIP_TR_SF6], "Csf6" }, { c.qnt_Cx, "Cx" } };
  for (int k = 0; k < MPHIP_NRADIO; k++) {
    if (q[k] < 0)
      continue;
    const std::string who = std::string("module_radio_decay: activity ") + names[k] + " (quantity " + std::to_string(q[k]) + ")";
    if (q[k] >= c.nq)
      return who + " is outside [0, nq = " + std::to_string(c.nq) + ")";
    for (int j = 0; j < k; j++)
      if (q[j] == q[k])
        return who + " is also activity " + names[j];
    for (const auto &t : taken)
      if (t.iq == q[k])
        return who + " is already quantity " + t.what;
    for (int m = 0; m < MPHIP_NMQ; m++)   // (module_meteo runs lazily, after the modules that write the activities)
      if (c.qnt_met[m] == q[k])
        return who + " is already a module_meteo quantity";
  }
  return "";
}

// chemistry in the step: the modules of chem_on, or module_tracer_chem (TRACER_CHEM; it alone does not run
// module_chem_grid)
bool step_chem_on(const mphip_ctl_t &c) {
  return chem_on(c) || c.tracer_chem != 0;
}

// ---- module_radio_depo ---------------------------------------------------------


// the deposition modules the control parameters configure (the bits of the step's tail, plan_step)
unsigned depo_bits(const mphip_ctl_t &c) {
  unsigned m = 0;
  if ((c.wet_depo_ic_a > 0 || c.wet_depo_ic_h[0] > 0) && (c.wet_depo_bc_a > 0 || c.wet_depo_bc_h[0] > 0))
    m |= MPHIP_MOD_WET_DEPO;
  if (c.dry_depo_vdep > 0)
    m |= MPHIP_MOD_DRY_DEPO;
  return m;
}

// the aerosol-bound activities: they deposit (the noble gases Rn-222 and Xe-133 never do)
constexpr int kRadioDepositing[kRadioDepoMax] = { MPHIP_RN_PB210, MPHIP_RN_BE7, MPHIP_RN_CS137, MPHIP_RN_I131 };

bool radio_depo_any(const RadioQnt &r) {
  for (int k : kRadioDepositing)
    if (r.q[k] >= 0)
      return true;
  return false;
}

// module_radio_depo in the step: the module is on, a depositing activity is registered and the wet or the dry module is
// configured.  Such a step takes the split path (the launch runs behind the tail, on the stored dt) and shares no
// multi-step launch.
bool step_radio_depo_on(const mphip_ctx *ctx) {
  return ctx->rdepo_on && radio_depo_any(ctx->radio) && depo_bits(ctx->ctl) != 0;
}

// what keeps module_radio_depo from being on under the control parameters c with the activities r ("" = nothing)
std::string radio_depo_conflict(const mphip_ctl_t &c, const RadioQnt &r) {
  if (c.direction != 1)
    return "module_radio_depo: DIRECTION must be 1 (the inventory of a backward run is not defined)";
  if (c.met_coord_type != 0)
    return "module_radio_depo: MET_COORD_TYPE must be 0 (longitude / latitude ground grid)";
  if (!radio_depo_any(r))
    return "module_radio_depo: no depositing activity (Apb210, Abe7, Acs137, Ai131) is registered with mphip_set_radio_decay";
  return "";
}

// One step of module_radio_depo at model time t: the ground decay of the inventory since its time, the particles'
// deposits (radio_depo_kernel), their sums per cell in ascending particle index (ordered_cell_sums), inv = inv f + step.
// busy: EmitKeys::depo_busy of the launch that moved the particles, if it holds for depo_bits' modules (NULL: the kernel
// decides from p, time and dt itself).
int launch_radio_depo(mphip_ctx *ctx, double t, const unsigned char *busy) {
  if (!ctx->d_rdepo_inv.p)
    return fail(ctx, "module_radio_depo: no ground grid (mphip_set_radio_depo)");
  const std::string why = radio_depo_conflict(ctx->ctl, ctx->radio);
  if (!why.empty())
    return fail(ctx, why);
  const mphip_ctl_t &c = ctx->ctl;
  const unsigned depo = depo_bits(c);
  const mphip_box_t &g = ctx->rdepo_grid;
  const size_t ntot = ctx->rdepo_ntot;
  RadioDepoArgs R;
  memset(&R, 0, sizeof(R));
  R.G = BoxGrid{ g.lon0, g.lon1, g.lat0, g.lat1, 0.0, 1.0, g.nx, g.ny, 1 };
  R.ncell = (int) (ntot - 1);
  RadioDepoAdd D;
  memset(&D, 0, sizeof(D));
  for (int k : kRadioDepositing)
    if (ctx->radio.q[k] >= 0) {
      R.q[R.ndep++] = ctx->radio.q[k];
      D.plane[D.ndep] = k;
      // (the C library's exp; first step: the inventory only gets its time)
      D.f[D.ndep++] = ctx->rdepo_have_t ? exp(-kRadioLambda[k] * (t - ctx->rdepo_t)) : 1.0;
    }
  const int nv = 2 * R.ndep;
  const double *step = nullptr;
  if (ctx->np > 0 && depo) {
    if (ctx->fused_perm)   // (never behind a step's tail: the launch that moved the particles has done the gather)
      return fail(ctx, "module_radio_depo: module_sort's gather of the particle arrays is still pending");
    if (ensure_packed(ctx) || check_fields(ctx, depo))
      return 1;
    if (ctx->force_generic || !lean32_ok(ctx))
      return fail(ctx, "module_radio_depo: needs the lean deposition code (a regular longitude / latitude meteo grid with a "
                       "pressure look-up table, packed records within 32-bit offsets, option generic_kernel off)");
    if (reserve(ctx, ctx->d_rec, (size_t) ctx->np * (size_t) nv) || reserve(ctx, ctx->d_sums, (size_t) nv * ntot))
      return 1;
    R.cell = ctx->d_cell.p;
    R.val = ctx->d_rec.p;
    StepParams S;
    memset(&S.emit, 0, sizeof(S.emit));
    S.ctl = c;
    S.met = dev_met(ctx);
    S.atm = dev_atm(ctx);
    S.clim = ctx->d_clim.p;
    S.tracers = ctx->d_tracers.p;
    S.t = t;
    S.mask = depo;
    // the partition of the deposition launch, with more blocks where the list of a block would not fit the LDS
    int blocks = ctx->step_blocks;
    BlockGeom geom = block_geom(ctx->np, blocks);
    const size_t axes = (axes_lds_bytes(ctx) + 15) & ~(size_t) 15;
    const size_t lds_max = 64 * 1024 - 8;   // (the kernel's own 8 B of static LDS come on top of the dynamic part)
    while (axes + (size_t) geom.per_block * sizeof(int) > lds_max && geom.per_block > 256) {
      blocks *= 2;
      geom = block_geom(ctx->np, blocks);
    }
    const size_t lds = axes + (size_t) geom.per_block * sizeof(int);
    if (lds > lds_max)
      return fail(ctx, "module_radio_depo: the axes of the meteo grid do not fit the LDS");
    S.nblocks_logical = geom.nblocks_logical;
    S.per_block = geom.per_block;
    S.xcd_map = ctx->xcd_map;
    S.depo_busy = busy;
    S.ctr_turb = S.ctr_meso = S.ctr_conv = S.ctr_pbl = 0;
    S.radio = ctx->radio;
    S.nsteps = 1;
    S.t_stride = 0;
    S.ctr_stride = 0;
    S.queue = nullptr;
    S.queue_n = S.queue_chunks = S.queue_waves = 0;
    hipEvent_t e1 = nullptr;
    if (prof_pair(ctx, ctx->stream, &e1))   // (mphip_profile_begin / _end: the kernel counts as a launch of the step)
      return 1;
    hipLaunchKernelGGL(radio_depo_kernel, dim3(geom.nblocks_logical), dim3(256), lds, ctx->stream, S, R);
    HIPCHK(hipGetLastError());
    if (ctx->prof)
      HIPCHK(hipEventRecord(e1, ctx->stream));
    const RecordVals vals = { ctx->d_rec.p, nv };
    if (ordered_cell_sums(ctx, vals, nv, 1, ntot, ctx->d_sums.p, (int *) nullptr, (double *) nullptr, true))
      return 1;
    step = ctx->d_sums.p;
  }
  // (behind the last refusal: a refused call leaves the inventory and its time as they were)
  ctx->rdepo_t = t;
  ctx->rdepo_have_t = true;
  if (D.ndep > 0) {
    hipLaunchKernelGGL(radio_depo_add_kernel, dim3(grid_for((long long) (2 * (size_t) D.ndep * ntot))), dim3(256), 0, ctx->stream,
                       ctx->d_rdepo_inv.p, step, ntot, D);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// the chemistry of a step, in the reference's order: module_chem_grid (with either chemistry; it does nothing without
// m or Cx), module_oh_chem, module_h2o2_chem, module_tracer_chem
int launch_chem(mphip_ctx *ctx, double t) {
  const mphip_ctl_t &c = ctx->ctl;
  return (chem_on(c)
          && (do_chem_grid(ctx, t) || (c.oh_chem_reaction != 0 && launch_oh(ctx))
              || (c.h2o2_chem_reaction != 0 && launch_h2o2(ctx))))
    || (c.tracer_chem != 0 && launch_tracer_chem(ctx));
}

// ---- the plan of a time step --------------------------------------------------

// what is due at model time t: module_sort (SORT_DT), module_mixing (MIXING_DT), module_convection (CONV_DT; every step
// without one) and module_meteo (MET_DT_OUT, mptrac.c:7921-7924)
struct StepDue {
  bool sort, mixing, conv, meteo;
};

StepDue due_at(const mphip_ctl_t &c, double t) {
  StepDue d;
  d.sort = c.sort_dt > 0 && fmod(t, c.sort_dt) == 0;
  d.mixing = c.mixing_trop >= 0 && c.mixing_strat >= 0 && (c.mixing_dt <= 0 || fmod(t, c.mixing_dt) == 0);
  d.conv = (c.conv_mix_pbl || c.conv_cape >= 0) && (c.conv_dt <= 0 || fmod(t, c.conv_dt) == 0);
  d.meteo = c.met_dt_out > 0 && (c.met_dt_out < c.dt_mod || fmod(t, c.met_dt_out) == 0);
  return d;
}

// the time step at t of mphip_run_timestep (mphip_run_timesteps takes the plan of a batch's first step for all of its
// steps: nothing is due in any of them)
struct StepPlan {
  StepDue due;
  unsigned mask;       // the launch that moves the particles
  unsigned tail;       // behind module_mixing and the chemistry: module_radio_decay, the deposition modules and the
                       // second call of module_bound_cond
  RngCtr rng;          // the counters of mask's module_rng calls, from ctx->rng_ctr on
  uint64_t per_step;   // ... and how far the step moves ctx->rng_ctr
};

StepPlan plan_step(const mphip_ctx *ctx, double t) {
  const mphip_ctl_t &c = ctx->ctl;
  StepPlan P;
  P.due = due_at(c, t);
  // (module_timesteps: do_sort's on a step that sorts)
  unsigned m = (P.due.sort ? 0u : MPHIP_MOD_TIMESTEPS) | MPHIP_MOD_POSITION | MPHIP_MOD_POSITION2;
  if (c.advect > 0)
    m |= MPHIP_MOD_ADVECT;
  if (c.diffusion
      && (c.turb_dx_pbl > 0 || c.turb_dz_pbl > 0 || c.turb_dx_trop > 0 || c.turb_dz_trop > 0 || c.turb_dx_strat > 0
          || c.turb_dz_strat > 0))
    m |= MPHIP_MOD_DIFF_TURB;
  if (c.diffusion && c.turb_pbl_scheme == 1)   // (between module_diff_turb and module_diff_meso, mptrac.c:7893-7901)
    m |= MPHIP_MOD_DIFF_PBL;
  if (c.diffusion && (c.turb_mesox > 0 || c.turb_mesoz > 0))
    m |= MPHIP_MOD_DIFF_MESO;
  if (P.due.conv)
    m |= MPHIP_MOD_CONVECTION;
  if (c.qnt_rp >= 0 && c.qnt_rhop >= 0)
    m |= MPHIP_MOD_SEDI;
  if (c.isosurf >= 1 && c.isosurf <= 4)
    m |= MPHIP_MOD_ISOSURF;
  const bool bound = c.bound_lat0 < c.bound_lat1 && c.bound_p0 > c.bound_p1;
  if (bound)
    m |= MPHIP_MOD_BOUND_COND;
  if (c.qnt_loss_rate >= 0)
    m |= MPHIP_MOD_LOSS_ZERO;
  if (c.tdec_trop > 0 && c.tdec_strat > 0)
    m |= MPHIP_MOD_DECAY;
  // module_radio_decay sits behind module_mixing and the chemistry: in the launch of the deposition modules
  unsigned tail = radio_step_bit(ctx);
  tail |= depo_bits(c);
  if (bound)
    tail |= MPHIP_MOD_BOUND_COND2;
  P.mask = m;
  P.tail = tail;
  P.rng = rng_counters(m, (uint64_t) ctx->np_total, ctx->rng_ctr, &P.per_step);
  return P;
}

// a deferred module_meteo of the step before, at the start of a step: dropped if this step runs module_meteo again
// (nobody saw its values), evaluated now -- before the particles move -- otherwise
int settle_meteo(mphip_ctx *ctx, bool meteo_due) {
  if (!meteo_due)
    return flush_meteo(ctx);
  ctx->meteo_pending = false;
  return 0;
}

void unpin_all(mphip_ctx *ctx, std::vector<std::pair<uintptr_t, uintptr_t>> &list) {
  std::lock_guard<std::mutex> guard(ctx->pinned_lock);
  for (auto &r : list)
    if (hipHostUnregister((void *) r.first) != hipSuccess)
      (void) hipGetLastError();
  list.clear();
}

// a host array of strides sx, sy holds a level field of ny x np values per column, a whole number of rows apart
bool regrid_strides_ok(int ny, int np, long long sx, long long sy) {
  return sy >= np && sx >= sy * ny && sx % sy == 0;
}

// levels of a level field and the strides of the host array that holds it
struct LevelField {
  int nlev;
  long long sx, sy;
};

// a level field of nx x ny x L.nlev values between such a host array and a compact device array (asynchronous on `stream`)
int copy3(mphip_ctx *ctx, hipStream_t stream, float *dev, const float *host, int nx, int ny, const LevelField &L, bool to_device) {
  const int np = L.nlev;
  const long long sx = L.sx, sy = L.sy;
  if (sy == np && sx == (long long) ny * np) {
    const size_t bytes = (size_t) nx * ny * np * sizeof(float);
    if (to_device)
      HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
    else
      HIPCHK(hipMemcpyAsync((void *) host, dev, bytes, hipMemcpyDeviceToHost, stream));
    return 0;
  }
  hipMemcpy3DParms p;
  memset(&p, 0, sizeof(p));
  const hipPitchedPtr h = make_hipPitchedPtr((void *) host, (size_t) sy * sizeof(float), (size_t) np, (size_t) (sx / sy));
  const hipPitchedPtr d = make_hipPitchedPtr(dev, (size_t) np * sizeof(float), (size_t) np, (size_t) ny);
  p.srcPtr = to_device ? h : d;
  p.dstPtr = to_device ? d : h;
  p.extent = make_hipExtent((size_t) np * sizeof(float), (size_t) ny, (size_t) nx);
  p.kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  HIPCHK(hipMemcpy3DAsync(&p, stream));
  return 0;
}

// a surface field of nx x ny values between a host array of row stride sx2 and a compact device array
int copy2(mphip_ctx *ctx, hipStream_t stream, float *dev, const float *host, int nx, int ny, long long sx2, bool to_device) {
  const size_t row = (size_t) ny * sizeof(float), hrow = (size_t) sx2 * sizeof(float);
  if (to_device)
    HIPCHK(hipMemcpy2DAsync(dev, row, host, hrow, row, (size_t) nx, hipMemcpyHostToDevice, stream));
  else
    HIPCHK(hipMemcpy2DAsync((void *) host, hrow, dev, row, row, (size_t) nx, hipMemcpyDeviceToHost, stream));
  return 0;
}

// ---- 16-bit packed level fields (mphip_pack.hpp) ------------------------------------------------------------------------
// is field f of a snapshot on model levels?
bool field_on_model_levels(int f) {
  return (f >= MPHIP_PL && f <= MPHIP_ZETA_DOTL) || f == MPHIP_WL;
}

// what is refused of a packed description whatever the call; NULL = accepted (`why` holds the message otherwise)
const char *packed_refusal(const mphip_met_packed_t *pk, std::string &why) {
  for (int f = 0; f < MPHIP_N3D; f++) {
    if (!pk->q3[f])
      continue;
    if (pk->base.f3[f])
      why = std::string("field ") + kField3Name[f] + " is given both as floats and as codes";
    else if (!pk->scl[f] || !pk->off[f])
      why = std::string("field ") + kField3Name[f] + " is given as codes without scl or off";
    else if (!(pk->lo[f] <= pk->hi[f]))
      why = std::string("field ") + kField3Name[f] + ": the limits need lo <= hi";
    else
      continue;
    return why.c_str();
  }
  return nullptr;
}

// LevelField of field f of a snapshot: npl levels (none if npl < 1) at sx_ml, sy_ml on model levels, else np at sx, sy;
// the strides are those of `arrays` where given (mphip_unpack_met: the grid is its input's, the arrays are its output's)
LevelField level_field(const mphip_met_t *met, int f, const mphip_met_t *arrays = nullptr) {
  const bool is_ml = field_on_model_levels(f);
  const mphip_met_t *a = arrays ? arrays : met;
  return LevelField{ is_ml ? std::max(met->npl, 0) : met->np, is_ml ? a->sx_ml : a->sx, is_ml ? a->sy_ml : a->sy };
}

// One field on the device on its way through a streaming kernel: {scl[nlev] | off[nlev]} doubles, then the codes, which
// keep their host array's offset from a 16-byte boundary (`shift` codes: the copy moves aligned runs to aligned runs, and
// the kernels' vector path starts where the codes are aligned).
struct PackedField {
  size_t n;                // values
  int nlev;
  size_t shift;            // codes in front of the first one, 0 ... 7
  size_t bytes;            // of the whole block
  char *blk;               // the block on the device, once its owner has one of `bytes` bytes
  double *scl() const { return (double *) blk; }
  double *off() const { return (double *) blk + nlev; }
  unsigned short *q() const { return (unsigned short *) (blk + 2 * (size_t) nlev * sizeof(double)) + shift; }
};

PackedField packed_field(size_t n, int nlev, const void *host_codes, char *blk = nullptr) {
  PackedField B;
  B.n = n;
  B.nlev = nlev;
  B.shift = ((uintptr_t) host_codes & 15) / sizeof(unsigned short);
  B.bytes = 2 * (size_t) nlev * sizeof(double) + (n + 2 * kPkVec) * sizeof(unsigned short);
  B.blk = blk;
  return B;
}

// grid, LDS and the scalar head of met_unpack_kernel / met_pack_quantise_kernel for n values whose codes start at q
struct PackStream {
  unsigned n, nlev, head;
  dim3 grid;
  size_t lds;
  bool table_in_lds;
};

PackStream pack_stream(const unsigned short *q, size_t n, int nlev) {
  PackStream P;
  P.n = (unsigned) n;
  P.nlev = (unsigned) nlev;
  P.head = (unsigned) std::min<size_t>(n, ((16 - ((uintptr_t) q & 15)) & 15) / sizeof(unsigned short));
  const size_t nvec = (n - P.head) / kPkVec;
  P.grid = dim3((unsigned) std::min<size_t>(std::max<size_t>((nvec + kPkThreads - 1) / kPkThreads, 1), kPkMaxBlocks));
  P.table_in_lds = nlev <= kPkLdsLevels;
  P.lds = P.table_in_lds ? 2 * (size_t) nlev * sizeof(double) : 0;
  return P;
}

// the host's scales, offsets and codes of field f into its block B (asynchronous on `stream`)
int upload_packed(mphip_ctx *ctx, hipStream_t stream, const PackedField &B, const mphip_met_packed_t *pk, int f) {
  HIPCHK(hipMemcpyAsync(B.scl(), pk->scl[f], (size_t) B.nlev * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(B.off(), pk->off[f], (size_t) B.nlev * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(B.q(), pk->q3[f], B.n * sizeof(unsigned short), hipMemcpyHostToDevice, stream));
  return 0;
}

// met_unpack_kernel of field f from its block B into dst; `launch` takes (kernel, grid, block, lds, arguments ...) and
// puts the kernel on its caller's stream in its caller's way
template <typename L>
int unpack_packed(const PackedField &B, const mphip_met_packed_t *pk, int f, float *dst, L launch) {
  const PackStream P = pack_stream(B.q(), B.n, B.nlev);
  return launch(P.table_in_lds ? met_unpack_kernel<true> : met_unpack_kernel<false>, P.grid, dim3(kPkThreads), P.lds,
                (const unsigned short *) B.q(), (const double *) B.scl(), (const double *) B.off(), dst, P.n, P.nlev, P.head,
                pk->lo[f], pk->hi[f]);
}

// the largest block a packed snapshot's fields need (0: no field is given as codes)
size_t packed_block_bytes(const mphip_met_packed_t *pk) {
  const mphip_met_t *met = &pk->base;
  size_t need = 0;
  for (int f = 0; f < MPHIP_N3D; f++) {
    const int nlev = level_field(met, f).nlev;
    if (pk->q3[f] && nlev > 0)
      need = std::max(need, packed_field((size_t) met->nx * met->ny * (size_t) nlev, nlev, pk->q3[f]).bytes);
  }
  return need;
}

// host -> device copies of one snapshot's fields into the staging arrays of slot S (asynchronous on `stream`); a field
// that `pk` gives as codes goes into the block `codes` (mphip_ctx::codes, reserved by the caller) and is decoded from there
// behind its copy
int upload_fields(mphip_ctx *ctx, MetSlot &S, const mphip_met_t *met, bool new_grid, hipStream_t stream,
                  const mphip_met_packed_t *pk = nullptr, char *codes = nullptr) {
  const size_t ncol = (size_t) met->nx * met->ny;
  auto launch = [&](auto kernel, dim3 grid, dim3 block, size_t lds, auto... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    HIPCHK(hipGetLastError());
    return 0;
  };
  for (int f = 0; f < MPHIP_N3D; f++) {
    const LevelField L = level_field(met, f);
    const bool coded = pk && pk->q3[f];
    S.has3[f] = (met->f3[f] != nullptr || coded) && L.nlev > 0;
    if (!S.has3[f])
      continue;
    const size_t n3 = ncol * (size_t) L.nlev;
    if (new_grid || !S.f3[f])
      HIPCHK(S.f3[f].resize(n3));
    if (coded) {
      const PackedField B = packed_field(n3, L.nlev, pk->q3[f], codes);
      if (upload_packed(ctx, stream, B, pk, f) || unpack_packed(B, pk, f, S.f3[f].p, launch))
        return 1;
      continue;
    }
    if (!regrid_strides_ok(met->ny, L.nlev, L.sx, L.sy))
      return fail(ctx, "unsupported 3-D meteo strides");
    if (copy3(ctx, stream, S.f3[f].p, met->f3[f], met->nx, met->ny, L, true))
      return 1;
  }
  S.ps11 = met->f2[MPHIP_PS] ? met->f2[MPHIP_PS][(size_t) met->sx2 + 1] : 0.f;
  S.ps_min = S.pct_min = S.pbl_min = S.pel_min = -HUGE_VAL;
  S.ps_max = S.pbl_max = HUGE_VAL;
  // smallest and largest value of a surface field if every value is finite
  auto extremes = [&](int f, double &lo_out, double &hi_out) {
    if (!met->f2[f])
      return;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int ix = 0; ix < met->nx; ix++)
      for (int iy = 0; iy < met->ny; iy++) {
        const float v = met->f2[f][(size_t) ix * (size_t) met->sx2 + iy];
        if (!std::isfinite(v))
          return;
        lo = std::min(lo, (double) v);
        hi = std::max(hi, (double) v);
      }
    lo_out = lo;
    hi_out = hi;
  };
  extremes(MPHIP_PS, S.ps_min, S.ps_max);
  extremes(MPHIP_PBL, S.pbl_min, S.pbl_max);
  if (met->f2[MPHIP_PEL]) {
    double lo = HUGE_VAL;
    for (int ix = 0; ix < met->nx; ix++)
      for (int iy = 0; iy < met->ny; iy++) {
        const float v = met->f2[MPHIP_PEL][(size_t) ix * (size_t) met->sx2 + iy];
        if (v == v)   // (a NaN never starts convection: dmin(ptop, NaN) is a NaN and p >= NaN is false)
          lo = std::min(lo, (double) v);
      }
    S.pel_min = lo;
  }
  if (met->f2[MPHIP_PCT]) {
    double lo = HUGE_VAL;
    for (int ix = 0; ix < met->nx; ix++)
      for (int iy = 0; iy < met->ny; iy++) {
        const float v = met->f2[MPHIP_PCT][(size_t) ix * (size_t) met->sx2 + iy];
        if (std::isfinite(v))
          lo = std::min(lo, (double) v);
      }
    if (lo < HUGE_VAL)
      S.pct_min = lo;
  }
  for (int f = 0; f < MPHIP_N2D; f++) {
    S.has2[f] = met->f2[f] != nullptr;
    if (!S.has2[f])
      continue;
    if (new_grid || !S.f2[f])
      HIPCHK(S.f2[f].resize(ncol));
    if (met->sx2 == met->ny) {
      HIPCHK(hipMemcpyAsync(S.f2[f].p, met->f2[f], ncol * sizeof(float), hipMemcpyHostToDevice, stream));
    } else {
      if (met->sx2 < met->ny)
        return fail(ctx, "unsupported 2-D meteo stride");
      HIPCHK(hipMemcpy2DAsync(S.f2[f].p, (size_t) met->ny * sizeof(float), met->f2[f], (size_t) met->sx2 * sizeof(float),
                              (size_t) met->ny * sizeof(float), (size_t) met->nx, hipMemcpyHostToDevice, stream));
    }
  }
  return 0;
}

// ---- mphip_derive_met, mphip_regrid_met, mphip_detrend_met, mphip_ingest_met, mphip_unpack_met, mphip_pack_met: what a
// ---- call of the six shares ----------------------------------------------------------------------------------------
// One call, from open() to the end of its scope: it holds the lock, hands out the scratch (PrepState), stages fields
// between the caller's arrays and that scratch (upload3 ... download2, uploads_complete), brackets what
// mphip_profile_begin / _end time with event pairs (tools/gpu_*_cost.py; a caller that profiles does not step from another
// thread) and, however the call ends, leaves nothing queued on the stream.  A copy may read the call's own vectors: those
// are declared before the PrepCall, so that they are destroyed after it.
struct PrepCall {
  mphip_ctx *ctx;
  PrepState &S;
  std::lock_guard<std::mutex> guard;
  hipStream_t st = nullptr;
  hipEvent_t ev_stop = nullptr;

  explicit PrepCall(mphip_ctx *c) : ctx(c), S(c->prep), guard(c->prep.lock) {}
  ~PrepCall() {
    if (st)
      (void) hipStreamSynchronize(st);
  }
  int open() {
    HIPCHK(hipSetDevice(ctx->device));
    if (!S.stream)
      HIPCHK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    st = S.stream;
    S.taken = 0;
    return 0;
  }
  // the end of an accepted call and of the event pair around its downloads: its results are in the caller's arrays
  int close() {
    if (mark_end())
      return 1;
    const hipStream_t s = st;
    st = nullptr;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
  }
  // the next buffer of the pool, for n > 0 values of T; NULL: the allocation failed (the buffer is empty then)
  template <typename T>
  T *take(size_t n) {
    if (S.taken == S.pool.size())
      S.pool.emplace_back();
    DevBuf<char> &b = S.pool[S.taken++];
    return reserve(ctx, b, n * sizeof(T)) ? nullptr : (T *) b.p;
  }
  // A field between the caller's array and a compact device array, on the call's stream: a level field of nx x ny columns
  // (L: its levels and the host array's strides) or a surface field (row stride sx2).  upload: into the next buffer of the
  // pool, which holds `room` values where that is more than the field's (mphip_ingest_met: the periodic column); NULL:
  // it failed.  to_device3: into a buffer taken earlier (the order of the takes decides which buffer serves what).
  float *upload3(const float *host, int nx, int ny, LevelField L, size_t room = 0) {
    float *const dev = take<float>(std::max(room, (size_t) nx * ny * L.nlev));
    return dev && !to_device3(dev, host, nx, ny, L) ? dev : nullptr;
  }
  float *upload2(const float *host, int nx, int ny, long long sx2, size_t room = 0) {
    float *const dev = take<float>(std::max(room, (size_t) nx * ny));
    return dev && !copy2(ctx, st, dev, host, nx, ny, sx2, true) ? dev : nullptr;
  }
  int to_device3(float *dev, const float *host, int nx, int ny, LevelField L) { return copy3(ctx, st, dev, host, nx, ny, L, true); }
  int download3(float *dev, float *host, int nx, int ny, LevelField L) { return copy3(ctx, st, dev, host, nx, ny, L, false); }
  int download2(float *dev, float *host, int nx, int ny, long long sx2) { return copy2(ctx, st, dev, host, nx, ny, sx2, false); }
  // The uploads are complete behind this.  With pageable memory the copies have read the caller's arrays when they
  // return; the synchronisation makes that hold for pinned arrays too, before the first download overwrites an input
  // that an output aliases, and it covers the call's own vectors that a copy reads.
  int uploads_complete() {
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // the axes of the output grid (taken before anything was written: `out` may alias `in`) into `out`, behind close()
  static void write_axes(const mphip_regrid_out_t *out, const std::vector<double> &lon2, const std::vector<double> &lat2,
                         const std::vector<double> &p2) {
    if (out->lon)
      memcpy(out->lon, lon2.data(), lon2.size() * sizeof(double));
    if (out->lat)
      memcpy(out->lat, lat2.data(), lat2.size() * sizeof(double));
    if (out->p)
      memcpy(out->p, p2.data(), p2.size() * sizeof(double));
  }
  // event pairs around every kernel (phase 0), around the uploads (1), around the downloads (2) or around the weight table
  // of mphip_detrend_met (3)
  int mark_begin(int phase) {
    ev_stop = nullptr;
    return ctx->derive_profile_phase == phase ? prof_pair(ctx, st, &ev_stop) : 0;
  }
  int mark_end() {
    if (ev_stop)
      HIPCHK(hipEventRecord(ev_stop, st));
    ev_stop = nullptr;
    return 0;
  }
  template <typename K, typename... Args>
  int enqueue(K kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // a kernel as one profiled event pair
  template <typename K, typename... Args>
  int launch(K kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    return mark_begin(0) || enqueue(kernel, grid, block, lds, args...) || mark_end();
  }
  // ... which a phase of its own singles out as well (4, 5, 6: the extremes, their reduction and the quantisation of
  // mphip_pack_met)
  template <typename K, typename... Args>
  int launch_as(int phase, K kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    return mark_begin(ctx->derive_profile_phase == phase ? phase : 0) || enqueue(kernel, grid, block, lds, args...) || mark_end();
  }
};

// columns per workgroup of a kernel that stages whole columns in lds_of(columns) bytes of LDS: the largest power of two up
// to kPrepLanes within 64 KB (0: not even one column fits)
template <typename F>
int columns_per_workgroup(F lds_of, size_t *lds) {
  for (int cpb = kPrepLanes; cpb >= 1; cpb >>= 1) {
    *lds = lds_of(cpb);
    if (*lds <= 64 * 1024)
      return cpb;
  }
  return 0;
}

// the refusals every call of the six makes of a grid; NULL = accepted
const char *grid_dims_refusal(int nx, int ny, bool axes_given = true) {
  return nx < 2 || ny < 2 || !axes_given ? "meteo grid dimensions out of range" : nullptr;
}

// nlev: the most levels a field of the call has
const char *grid_size_refusal(int nx, int ny, long long nlev) {
  return (long long) nx * ny >= (1LL << 24) || (long long) nx * ny * nlev >= (1LL << 31)
    ? "meteo grid too large for the device index arithmetic" : nullptr;
}

// ... of a pressure-level grid, in the order the calls report them
const char *grid_refusal(int nx, int ny, int np, bool axes_given = true) {
  if (const char *why = grid_dims_refusal(nx, ny, axes_given))
    return why;
  if (np < 2)
    return "needs two pressure levels or more (np < 2)";
  return grid_size_refusal(nx, ny, np);
}

// ---- mphip_regrid_met: the checks it shares with mphip_regrid_shape --------------------------------------------------

// the fields ML2PL regrids; SAMPLE takes these and z, pv
const int kRegridMl[kRgFields] = { MPHIP_T, MPHIP_U, MPHIP_V, MPHIP_W, MPHIP_H2O, MPHIP_O3, MPHIP_LWC, MPHIP_RWC,
                                   MPHIP_IWC, MPHIP_SWC, MPHIP_CC };
const int kRegridPl[kRgFields + 2] = { MPHIP_T, MPHIP_U, MPHIP_V, MPHIP_W, MPHIP_H2O, MPHIP_O3, MPHIP_LWC, MPHIP_RWC,
                                       MPHIP_IWC, MPHIP_SWC, MPHIP_CC, MPHIP_Z, MPHIP_PV };

struct RegridPlan {
  int nx, ny, np0;         // input extents (np0: levels of the uploaded level fields)
  int np1;                 // levels SAMPLE reads: met_np behind ML2PL, else np0
  int nx2, ny2, np2;       // output extents
  int ml_cpb;              // ML2PL: columns per workgroup
  size_t ml_lds;
  RegridSample S3, S2;     // SAMPLE: the level fields and the surface fields
  size_t lds3, lds2;
};

// everything that can be refused for the grid and the options (not for missing arrays); NULL = accepted
const char *regrid_plan(const mphip_met_t *in, unsigned what, const mphip_regrid_t *opt, RegridPlan *P) {
  const bool ml = what & MPHIP_REGRID_ML2PL, sample = what & MPHIP_REGRID_SAMPLE;
  if (!what || (what & ~(unsigned) (MPHIP_REGRID_ML2PL | MPHIP_REGRID_SAMPLE)))
    return "`what` must be an OR of MPHIP_REGRID_* bits";
  // (ML2PL has refusals of its own for the levels, between those of the dimensions and of the size)
  if (const char *why = ml ? grid_dims_refusal(in->nx, in->ny) : grid_refusal(in->nx, in->ny, in->np))
    return why;
  memset(P, 0, sizeof(*P));
  P->nx = in->nx;
  P->ny = in->ny;
  P->np0 = P->np1 = in->np;
  if (ml) {
    if (in->npl < 2 || in->np != in->npl)
      return "MPHIP_REGRID_ML2PL needs two model levels or more and np == npl";
    if (opt->met_np < 2 || !opt->met_p)
      return "MPHIP_REGRID_ML2PL needs two target levels or more (met_np < 2)";
    for (int j = 0; j < opt->met_np; j++)
      if (!(opt->met_p[j] > 0 && opt->met_p[j] < INFINITY) || (j > 0 && !(opt->met_p[j] < opt->met_p[j - 1])))
        return "MPHIP_REGRID_ML2PL: met_p must be finite, positive and strictly descending";
    const size_t pitch = in->npl | 1;
    P->ml_cpb = columns_per_workgroup(
      [&](int cpb) { return (size_t) opt->met_np * sizeof(double) + cpb * pitch * sizeof(float); }, &P->ml_lds);
    if (!P->ml_cpb)
      return "MPHIP_REGRID_ML2PL: too many levels for one column in 64 KB of LDS";
    P->np1 = opt->met_np;
    if (const char *why = grid_size_refusal(in->nx, in->ny, std::max(P->np0, P->np1)))
      return why;
  }
  P->nx2 = in->nx;
  P->ny2 = in->ny;
  P->np2 = P->np1;
  if (sample) {
    const int d[3] = { opt->met_dx, opt->met_dy, opt->met_dp }, s[3] = { opt->met_sx, opt->met_sy, opt->met_sp };
    for (int a = 0; a < 3; a++)
      if (d[a] < 1 || s[a] < 1)
        return "MPHIP_REGRID_SAMPLE: every stride and half-width must be 1 or more";
    if (s[0] - 1 > in->nx)
      return "MPHIP_REGRID_SAMPLE: smoothing half-width too large (met_sx - 1 <= nx)";
    // (the extents in 64 bits, and a half-width beyond 2^20 refused at once: no overflow for absurd options)
    const int n1[3] = { in->nx, in->ny, P->np1 }, tile[3] = { kRgTX, kRgTY, kRgKC };
    long long e[3], h[3];
    int n2[3];
    for (int a = 0; a < 3; a++) {
      n2[a] = (int) (((long long) n1[a] + d[a] - 1) / d[a]);
      if (s[a] > (1 << 20))
        return "MPHIP_REGRID_SAMPLE: smoothing tile with halo beyond 64 KB of LDS";
      e[a] = std::min<long long>(d[a], 2LL * s[a] - 1);
      h[a] = (tile[a] - 1) * e[a] + 2LL * s[a] - 1;
    }
    if (n2[0] < 2 || n2[1] < 2 || n2[2] < 2)
      return "MPHIP_REGRID_SAMPLE: the sampled grid needs two points or more per axis";
    if (h[0] * h[1] > 16 * 1024 || h[0] * h[1] * h[2] > 16 * 1024)
      return "MPHIP_REGRID_SAMPLE: smoothing tile with halo beyond 64 KB of LDS";
    P->nx2 = n2[0];
    P->ny2 = n2[1];
    P->np2 = n2[2];
    RegridSample &S = P->S3;
    S.nx = n1[0], S.ny = n1[1], S.np = n1[2];
    S.nx2 = n2[0], S.ny2 = n2[1], S.np2 = n2[2];
    S.dx = d[0], S.dy = d[1], S.dp = d[2];
    S.sx = s[0], S.sy = s[1], S.sp = s[2];
    S.ex = (int) e[0], S.ey = (int) e[1], S.ep = (int) e[2];
    S.hx = (int) h[0], S.hy = (int) h[1], S.hk = (int) h[2];
    P->lds3 = (size_t) (h[0] * h[1] * h[2]) * sizeof(float);
    P->S2 = S;
    P->S2.np = P->S2.np2 = P->S2.dp = P->S2.sp = P->S2.ep = P->S2.hk = 1;
    P->lds2 = (size_t) (h[0] * h[1]) * sizeof(float);
  }
  return nullptr;
}

// ---- mphip_detrend_met: the checks and the weight table -------------------------------------------------------------
const int kDetrendFields[kDtFields] = { MPHIP_T, MPHIP_U, MPHIP_V, MPHIP_W };

struct DetrendPlan {
  int nx, ny, np, sy, nchunk;
  double tssq, dlon;
  std::vector<DetrendRow> rows;      // (ws is filled by detrend_weights)
  size_t nw;                         // floats of the table
  double taps_mean;                  // window sizes over the rows
  long long taps_max;
};

// everything that can be refused for the grid and the option (the axes are there); NULL = accepted
const char *detrend_plan(const mphip_met_t *in, const mphip_detrend_t *opt, DetrendPlan *P) {
#pragma clang fp contract(off)
  if (const char *why = grid_refusal(in->nx, in->ny, in->np))
    return why;
  if (in->coord_type != 0)
    return "needs a longitude / latitude grid (coord_type != 0)";
  if (!(opt->met_detrend > 0 && opt->met_detrend < INFINITY))
    return "met_detrend must be finite and positive";
  const double dlon = fabs(in->lon[1] - in->lon[0]), dlat = fabs(in->lat[1] - in->lat[0]);
  if (!(dlon > 0 && dlon < INFINITY) || !(dlat > 0 && dlat < INFINITY))
    return "the grid spacing (dlon, dlat) must be finite and not zero";
  const int nx = in->nx, ny = in->ny;
  P->nx = nx;
  P->ny = ny;
  P->np = in->np;
  P->dlon = dlon;
  const double sigma = opt->met_detrend / 2.355;
  P->tssq = 2. * sigma * sigma;
  // (the limits are applied before the conversion to int: a quotient beyond the int range is the upper limit)
  auto half_width = [](double v, int hi) {
    const int s = !(v < hi) ? hi : (int) v;
    return s < 1 ? 1 : s;
  };
  const double dy_deg = sigma * 180. / (M_PI * 6367.421);                                      // DY2DEG(sigma)
  P->sy = half_width(3. * dy_deg / dlat, ny / 2);
  const long long ngroup = (nx + kDtTX - 1) / kDtTX;
  P->nchunk = (int) ((ngroup * in->np + kDtThreads - 1) / kDtThreads);
  if ((long long) P->nchunk * ny >= (1LL << 31))
    return "meteo grid too large for the device index arithmetic";
  P->rows.resize((size_t) ny);
  size_t nw = 0;
  double taps = 0;
  P->taps_max = 0;
  for (int iy = 0; iy < ny; iy++) {
    const double lat = in->lat[iy];
    const double dx_deg = (lat < -89.999 || lat > 89.999) ? 0. : sigma * 180. / (M_PI * 6367.421 * cos(lat * (M_PI / 180.0)));
    DetrendRow &R = P->rows[(size_t) iy];
    R.sx = half_width(3. * dx_deg / dlon, nx / 2);
    R.ylo = std::max(iy - P->sy, 0);
    R.nr = std::min(iy + P->sy, ny - 1) - R.ylo + 1;
    R.off = (long long) nw;
    R.ws = 0.f;
    nw += (size_t) R.nr * (size_t) (R.sx + 1);
    const long long t = (long long) R.nr * (2LL * R.sx + 1);
    taps += (double) t;
    P->taps_max = std::max(P->taps_max, t);
  }
  P->nw = nw + kDtTX;      // (padding: the kernel loads kDtTX entries at a time and ignores those beyond a row)
  P->taps_mean = taps / ny;
  return nullptr;
}

// the weights of the rows [iy0, iy1) and their sums: double arithmetic with the host's C library, each weight rounded to
// float once; ws by serial float additions in the order of the stencil's loops (ix2 ascending, iy2 ascending inside)
void detrend_weights(const DetrendPlan &P, const double *cphi, const double *sphi, const double *clam, const double *slam,
                     int iy0, int iy1, DetrendRow *rows, float *w) {
#pragma clang fp contract(off)
  const double re = 6367.421 + 0.0;
  for (int iy = iy0; iy < iy1; iy++) {
    DetrendRow &R = rows[iy];
    float *wr = w + R.off;
    const double x0[3] = { re * cphi[iy] * clam[0], re * cphi[iy] * slam[0], re * sphi[iy] };
    for (int r = 0; r < R.nr; r++) {
      const int iy2 = R.ylo + r;
      for (int d = 0; d <= R.sx; d++) {
        const double x1[3] = { re * cphi[iy2] * clam[d], re * cphi[iy2] * slam[d], re * sphi[iy2] };
        const double d2 = (x0[0] - x1[0]) * (x0[0] - x1[0]) + (x0[1] - x1[1]) * (x0[1] - x1[1])
          + (x0[2] - x1[2]) * (x0[2] - x1[2]);
        wr[(size_t) r * (R.sx + 1) + d] = (float) exp(-d2 / P.tssq);
      }
    }
    float ws = 0.f;
    for (int e = -R.sx; e <= R.sx; e++)
      for (int r = 0; r < R.nr; r++)
        ws = ws + wr[(size_t) r * (R.sx + 1) + (e < 0 ? -e : e)];
    R.ws = ws;
  }
}

void detrend_table(const mphip_met_t *in, DetrendPlan &P, std::vector<float> &w) {
#pragma clang fp contract(off)
  const int ny = P.ny, nd = P.nx / 2 + 1;
  std::vector<double> cphi((size_t) ny), sphi((size_t) ny), clam((size_t) nd), slam((size_t) nd);
  for (int iy = 0; iy < ny; iy++) {
    const double phi = in->lat[iy] * (M_PI / 180.0);
    cphi[(size_t) iy] = cos(phi);
    sphi[(size_t) iy] = sin(phi);
  }
  for (int d = 0; d < nd; d++) {
    const double lam = ((double) d * P.dlon) * (M_PI / 180.0);
    clam[(size_t) d] = cos(lam);
    slam[(size_t) d] = sin(lam);
  }
  w.resize(P.nw);
  // the rows are independent: a large table is built by a few threads, each on rows of about equal table share
  const int nthreads = P.nw < (1u << 20) ? 1 : 8;
  std::vector<std::thread> pool;
  int iy0 = 0;
  for (int t = 0; t < nthreads; t++) {
    int iy1 = iy0;
    const size_t upto = P.nw / nthreads * (size_t) (t + 1);
    while (iy1 < ny && (t == nthreads - 1 || (size_t) P.rows[(size_t) iy1].off < upto))
      iy1++;
    if (t == nthreads - 1)
      detrend_weights(P, cphi.data(), sphi.data(), clam.data(), slam.data(), iy0, iy1, P.rows.data(), w.data());
    else if (iy1 > iy0)
      pool.emplace_back([&, iy0, iy1] {
        detrend_weights(P, cphi.data(), sphi.data(), clam.data(), slam.data(), iy0, iy1, P.rows.data(), w.data());
      });
    iy0 = iy1;
  }
  for (auto &th : pool)
    th.join();
}

}   // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

size_t mphip_sizeof_ctl(void) {
  return sizeof(mphip_ctl_t);
}

size_t mphip_sizeof_met(void) {
  return sizeof(mphip_met_t);
}

size_t mphip_sizeof_prep(void) {
  return sizeof(mphip_prep_t);
}

const char *mphip_version(void) {
#if MPHIP_EXACT_DIV
  return "mptrac_amd 0.1 (gfx950, reference rounding)";   // libmptrac_hip_exact.so (mptrac_amd/build.py:EXACT_FLAGS)
#else
  return "mptrac_amd 0.1 (gfx950)";
#endif
}

int mphip_create(mphip_ctx **out, int device) {
  if (!out)
    return 1;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fprintf(stderr, "mptrac_hip: no HIP device available (this back end has no CPU fallback)\n");
    return 2;
  }
  if (device < 0 || device >= ndev) {
    fprintf(stderr, "mptrac_hip: device %d out of range (%d devices)\n", device, ndev);
    return 3;
  }
  mphip_ctx *ctx = new mphip_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    fprintf(stderr, "mptrac_hip: cannot initialise device %d\n", device);
    delete ctx;
    return 4;
  }
  memset(&ctx->ctl, 0, sizeof(ctx->ctl));
  *out = ctx;
  return 0;
}

// What is not memory ends here, every stream synchronised first; the buffers free themselves with the context.
void mphip_destroy(mphip_ctx *ctx) {
  if (!ctx)
    return;
  (void) hipSetDevice(ctx->device);
  (void) hipStreamSynchronize(ctx->stream);
  if (ctx->comm)
    (void) rccl().CommDestroy(ctx->comm);
  if (ctx->uploader.joinable())
    ctx->uploader.join();
  for (hipStream_t s : { ctx->copy_stream, ctx->ahead_stream, ctx->prep.stream })
    if (s) {
      (void) hipStreamSynchronize(s);
      (void) hipStreamDestroy(s);
    }
  for (hipEvent_t e : { ctx->next_ready, ctx->main_mark, ctx->ahead_mark, ctx->ahead_done, ctx->sel_copied[0], ctx->sel_copied[1] })
    if (e)
      (void) hipEventDestroy(e);
  for (auto e : ctx->ev)
    (void) hipEventDestroy(e);
  unpin_all(ctx, ctx->pinned);
  (void) hipStreamDestroy(ctx->stream);
  (void) hipSetDevice(ctx->device);
  delete ctx;
}

const char *mphip_last_error(const mphip_ctx *ctx) {
  return ctx ? ctx->err.c_str() : "no context";
}

int mphip_update_ctl(mphip_ctx *ctx, const mphip_ctl_t *ctl) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx || !ctl)
    return fail(ctx, "null argument");
  if (ctl->nq < 0 || ctl->nq > MPHIP_NQ_MAX)
    return fail(ctx, "nq out of range");
  if (ctl->rng_type != 1)
    return fail(ctx, "only RNG_TYPE 1 (Squares) is implemented on the device");
  if (ctl->advect_vert_coord < 0 || ctl->advect_vert_coord > 3)
    return fail(ctx, "Set ADVECT_VERT_COORD to 0, 1, 2, or 3!");
  if (!(ctl->advect == 0 || ctl->advect == 1 || ctl->advect == 2 || ctl->advect == 4))
    return fail(ctx, "Set ADVECT to 1, 2, or 4!");
  if (ctl->oh_chem_reaction < 0 || ctl->oh_chem_reaction > 3)   // (the reference would compute NaN masses)
    return fail(ctx, "Set OH_CHEM_REACTION to 0, 1, 2, or 3!");
  // module_meteo runs after the loss / mixing / deposition modules here and is evaluated lazily: none of the
  // quantities it fills may be one those modules read or write
  for (int k = 0; k < MPHIP_NMQ; k++)
    if (ctl->qnt_met[k] >= 0)
      for (int other : { ctl->qnt_m, ctl->qnt_vmr, ctl->qnt_aoa, ctl->qnt_loss_rate, ctl->qnt_mloss_decay,
                         ctl->qnt_mloss_wet, ctl->qnt_mloss_dry, ctl->qnt_mloss_oh, ctl->qnt_mloss_h2o2, ctl->qnt_Cx,
                         ctl->qnt_rp, ctl->qnt_rhop, ctl->qnt_ens,
                         ctl->qnt_zeta, ctl->qnt_eta, ctl->qnt_tracer[0], ctl->qnt_tracer[1], ctl->qnt_tracer[2],
                         ctl->qnt_tracer[3], ctl->qnt_tracer[4] })
        if (ctl->qnt_met[k] == other)
          return fail(ctx, "a module_meteo quantity shares its index with a mass / mixing-ratio / loss / particle quantity");
  if (radio_any(ctx)) {   // the activities of mphip_set_radio_decay stay valid under the new parameters
    const std::string why = radio_conflict(*ctl, ctx->radio.q);
    if (!why.empty())
      return fail(ctx, why);
  }
  if (ctx->rdepo_on) {    // ... and so does a module_radio_depo that is on
    const std::string why = radio_depo_conflict(*ctl, ctx->radio);
    if (!why.empty())
      return fail(ctx, why);
  }
  if (ctx->have_ctl && flush_meteo(ctx))   // a deferred module_meteo belongs to the old parameters
    return 1;
  if (!ctx->have_ctl || ctx->ctl.advect_vert_coord != ctl->advect_vert_coord)
    ctx->packed_dirty = true;               // the model-level wind records carry zeta_dot or omega
  // module_chem_grid's tables, with the C library's exp and cos as the reference computes them: pressures of the level
  // centres P(z0 + dz (iz + 0.5)), the cell areas dlat dlon (RE pi / 180)^2 cos(lat), the cell centres; built when the
  // grid will run and is valid (do_chem_grid refuses an invalid one)
  ctx->chemgrid_ok = false;
  if (chem_on(*ctl) && ctl->qnt_m >= 0 && ctl->qnt_Cx >= 0 && chemgrid_valid(*ctl)) {
    const int nx = ctl->chemgrid_nx, ny = ctl->chemgrid_ny, nz = ctl->chemgrid_nz;
    const double dz = (ctl->chemgrid_z1 - ctl->chemgrid_z0) / nz;
    const double dlon = (ctl->chemgrid_lon1 - ctl->chemgrid_lon0) / nx;
    const double dlat = (ctl->chemgrid_lat1 - ctl->chemgrid_lat0) / ny;
    std::vector<double> tab((size_t) nz + 2 * (size_t) ny + nx);
    double *press = tab.data(), *area = press + nz, *lon = area + ny, *lat = lon + nx;
    for (int iz = 0; iz < nz; iz++)
      press[iz] = kP0 * exp(-(ctl->chemgrid_z0 + dz * (iz + 0.5)) / kH0);
    for (int ix = 0; ix < nx; ix++)
      lon[ix] = ctl->chemgrid_lon0 + dlon * (ix + 0.5);
    for (int iy = 0; iy < ny; iy++) {
      lat[iy] = ctl->chemgrid_lat0 + dlat * (iy + 0.5);
      area[iy] = dlat * dlon * ((kRE * M_PI / 180.) * (kRE * M_PI / 180.)) * cos(lat[iy] * M_PI / 180.);
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the old tables may still be read)
    HIPCHK(ctx->d_chemgrid.resize(tab.size()));
    HIPCHK(hipMemcpy(ctx->d_chemgrid.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->chemgrid_ok = true;
  }
  ctx->h2o2_low = pow(1. / kH2O2CorA, 1. / kH2O2CorB);
  ctx->ctl = *ctl;
  ctx->have_ctl = true;
  return 0;
}

int mphip_update_clim(mphip_ctx *ctx, int ntime, int nlat, const double *tropo_time, const double *tropo_lat,
                      const double *tropo, int ld) {
  if (!ctx || !tropo_time || !tropo_lat || !tropo)
    return fail(ctx, "null argument");
  if (ntime < 2 || ntime > 12 || nlat < 2 || nlat > 73 || ld < nlat)
    return fail(ctx, "tropopause climatology dimensions out of range");
  HIPCHK(hipSetDevice(ctx->device));
  DevClim h;
  memset(&h, 0, sizeof(h));
  h.ntime = ntime;
  h.nlat = nlat;
  for (int i = 0; i < ntime; i++)
    h.time[i] = tropo_time[i];
  for (int j = 0; j < nlat; j++)
    h.lat[j] = tropo_lat[j];
  for (int i = 0; i < ntime; i++)
    for (int j = 0; j < nlat; j++)
      h.tropo[i][j] = tropo[(size_t) i * ld + j];
  for (int i = 0; i + 1 < ntime; i++)
    h.inv_dtime[i] = 1.0 / (h.time[i + 1] - h.time[i]);
  for (int j = 0; j + 1 < nlat; j++)
    h.inv_dlat[j] = 1.0 / (h.lat[j + 1] - h.lat[j]);
  HIPCHK(ctx->d_clim.reserve(1));
  HIPCHK(hipMemcpyAsync(ctx->d_clim.p, &h, sizeof(DevClim), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->h_clim = h;
  ctx->have_clim = true;
  return 0;
}

int mphip_update_clim_zm(mphip_ctx *ctx, int which, int ntime, int np, int nlat, const double *time, const double *p,
                         const double *lat, const double *vmr) {
  if (!ctx || which < 0 || which >= MPHIP_NZM)
    return fail(ctx, "bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))   // (a deferred module_meteo reads the tables of its own step)
    return 1;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->d_zm[which].release();
  memset(&ctx->zm[which], 0, sizeof(DevZm));
  if (ntime == 0)
    return 0;
  if (!time || !p || !lat || !vmr)
    return fail(ctx, "null argument");
  if (ntime < 2 || np < 2 || nlat < 2 || ntime > 4096 || np > 4096 || nlat > 4096)
    return fail(ctx, "climatology dimensions out of range");
  if (!(p[0] > p[1]))
    return fail(ctx, "Pressure data are not descending!");      // messages of read_clim_zm, mptrac.c:8768, 8774
  if (!(lat[0] < lat[1]))
    return fail(ctx, "Latitude data are not ascending!");
  const size_t nv = (size_t) ntime * (size_t) np * (size_t) nlat, n = (size_t) ntime + np + nlat + nv;
  HIPCHK(ctx->d_zm[which].resize(n));
  double *d = ctx->d_zm[which].p;
  HIPCHK(hipMemcpy(d, time, (size_t) ntime * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + ntime, p, (size_t) np * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + ntime + np, lat, (size_t) nlat * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + ntime + np + nlat, vmr, nv * sizeof(double), hipMemcpyHostToDevice));
  DevZm &z = ctx->zm[which];
  z.time = d;
  z.p = d + ntime;
  z.lat = d + ntime + np;
  z.vmr = d + ntime + np + nlat;
  z.ntime = ntime;
  z.np = np;
  z.nlat = nlat;
  return 0;
}

int mphip_update_clim_photo(mphip_ctx *ctx, int np, int nsza, int no3c, const double *p, const double *sza,
                            const double *o3c, const double *const rate[MPHIP_NTR]) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))
    return 1;
  HIPCHK(hipStreamSynchronize(ctx->stream));   // (kernels in flight may read the old tables)
  ctx->d_photo.release();
  memset(&ctx->photo, 0, sizeof(DevPhoto));
  for (bool &h : ctx->photo_have)
    h = false;
  if (np == 0)
    return 0;
  if (!p || !sza || !o3c || !rate)
    return fail(ctx, "null argument");
  if (rate[MPHIP_TR_SF6])
    return fail(ctx, "photolysis rates: SF6 has no table (rate[MPHIP_TR_SF6] must be NULL)");
  if (np < 2 || nsza < 2 || no3c < 2 || np > 4096 || nsza > 4096 || no3c > 4096
      || (size_t) np * (size_t) nsza * (size_t) no3c > ((size_t) 1 << 26))
    return fail(ctx, "photolysis rates: dimensions out of range");
  for (int i = 1; i < np; i++)        // (messages of the reference's reader)
    if (!(p[i] < p[i - 1]))
      return fail(ctx, "Pressure data are not descending!");
  for (int i = 1; i < nsza; i++)
    if (!(sza[i] > sza[i - 1]))
      return fail(ctx, "Solar zenith angle data are not ascending!");
  for (int i = 1; i < no3c; i++)
    if (!(o3c[i] > o3c[i - 1]))
      return fail(ctx, "Total column ozone data are not ascending!");
  // [p | sza | o3c], padded to whole records, then the interleaved rates
  const size_t nrec = (size_t) np * nsza * no3c, naxes = ((size_t) np + nsza + no3c + 3) / 4 * 4;
  std::vector<double> h(naxes + 4 * nrec, 0.0);
  std::copy(p, p + np, h.begin());
  std::copy(sza, sza + nsza, h.begin() + np);
  std::copy(o3c, o3c + no3c, h.begin() + np + nsza);
  for (int k = 0; k < 4; k++)
    if (rate[k])
      for (size_t j = 0; j < nrec; j++)
        h[naxes + 4 * j + k] = rate[k][j];
  HIPCHK(ctx->d_photo.resize(h.size()));
  double *d = ctx->d_photo.p;
  HIPCHK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  DevPhoto &ph = ctx->photo;
  ph.p = d;
  ph.sza = d + np;
  ph.o3c = d + np + nsza;
  ph.rec = (const PhotoRec *) (d + naxes);
  ph.np = np;
  ph.nsza = nsza;
  ph.no3c = no3c;
  for (int k = 0; k < 4; k++)
    ctx->photo_have[k] = rate[k] != nullptr;
  return 0;
}

int mphip_update_clim_ts(mphip_ctx *ctx, int which, int ntime, const double *time, const double *vmr) {
  if (!ctx || which < 0 || which >= MPHIP_NTR)
    return fail(ctx, "bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (ahead_drop(ctx))
    return 1;
  HIPCHK(hipStreamSynchronize(ctx->stream));   // kernels in flight may read the old series
  ctx->d_ts[which].release();
  DevTracerSeries &h = ctx->h_tracers;
  h.time[which] = h.vmr[which] = nullptr;
  h.ntime[which] = 0;
  if (ntime != 0) {
    if (!time || !vmr)
      return fail(ctx, "null argument");
    if (ntime < 2)
      return fail(ctx, "Not enough data points!");                 // messages of read_clim_ts, mptrac.c:8712-8730
    for (int i = 1; i < ntime; i++)
      if (!(time[i] > time[i - 1]))
        return fail(ctx, "Time series must be ascending!");
    HIPCHK(ctx->d_ts[which].resize(2 * (size_t) ntime));
    double *d = ctx->d_ts[which].p;
    HIPCHK(hipMemcpy(d, time, (size_t) ntime * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + ntime, vmr, (size_t) ntime * sizeof(double), hipMemcpyHostToDevice));
    h.time[which] = d;
    h.vmr[which] = d + ntime;
    h.ntime[which] = ntime;
  }
  HIPCHK(ctx->d_tracers.reserve(1));
  HIPCHK(hipMemcpy(ctx->d_tracers.p, &h, sizeof(DevTracerSeries), hipMemcpyHostToDevice));
  return 0;
}

// mphip_update_met, and mphip_update_met_packed (pk: the description `met` is the base of)
static int update_met_any(mphip_ctx *ctx, int slot, const mphip_met_t *met, const mphip_met_packed_t *pk) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx || !met || slot < 0 || slot > 1)
    return fail(ctx, "bad argument");
  std::string why;
  if (pk && packed_refusal(pk, why))
    return fail(ctx, "mphip_update_met_packed: " + why);
  if (met->nx < 2 || met->ny < 2 || met->np < 2 || !met->lon || !met->lat || !met->p)
    return fail(ctx, "meteo grid dimensions out of range");
  // index arithmetic of the kernels (cell_of / col_of): 24-bit factors, 31-bit cell index
  if ((long long) met->nx * met->ny >= (1LL << 24) || (long long) met->nx * met->ny * std::max(met->np, met->npl) >= (1LL << 31)
      || met->np >= (1 << 24))
    return fail(ctx, "meteo grid too large for the device index arithmetic");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))   // a deferred module_meteo samples the snapshots it was scheduled with
    return 1;
  const int nml = met->npl > 0 ? met->npl : 0;
  const bool new_grid = (met->nx != ctx->nx || met->ny != ctx->ny || met->np != ctx->npl || nml != ctx->nml);
  if (new_grid) {
    if (ctx->slot[0].valid || ctx->slot[1].valid) {
      // mptrac_get_met: "Meteo grid dimensions do not match!" (mptrac.c:6543-6546)
      if (ctx->slot[(slot ^ 1) ^ ctx->flip].valid)
        return fail(ctx, "Meteo grid dimensions do not match!");
    }
    ctx->nx = met->nx;
    ctx->ny = met->ny;
    ctx->npl = met->np;
    ctx->nml = nml;
    if (ctx->uploader.joinable())
      ctx->uploader.join();
    if (ctx->copy_stream)
      HIPCHK(hipStreamSynchronize(ctx->copy_stream));
    for (auto &q : ctx->next.f3)
      q.release();
    for (auto &q : ctx->next.f2)
      q.release();
    for (auto &b : ctx->codes)   // (idle: every upload into a slot ends with its stream synchronised, the uploader was joined)
      b.release();
    ctx->next.valid = false;
    ctx->next_pending = false;
    ctx->pk = mphip_ctx::PackedGrids();
    ctx->pk_next = mphip_ctx::PackedGrids();
    ctx->pk_next_valid = false;
  }
  if (ctx->next_pending) {   // a snapshot uploaded now changes what the prefetched pair would have been packed from
    if (ctx->uploader.joinable())
      ctx->uploader.join();
    HIPCHK(hipStreamSynchronize(ctx->copy_stream));
    ctx->pk_next_valid = false;
  }
  ctx->coord_type = met->coord_type;
  MetSlot &S = ctx->slot[slot ^ ctx->flip];
  S.lon.assign(met->lon, met->lon + met->nx);
  S.lat.assign(met->lat, met->lat + met->ny);
  S.p.assign(met->p, met->p + met->np);
  // the reference interpolates on met0's axes (mptrac.c:3010-3020); slot 0 defines them
  if (slot == 0 || new_grid || ctx->h_lon.empty()) {
    ctx->h_lon = S.lon;
    ctx->h_lat = S.lat;
    ctx->h_p = S.p;
    if (upload_axes(ctx))
      return 1;
    // an axis that passes for periodic and still leaves a gap: the early exits are off (dev_met), which costs time only
    const double first = ctx->h_lon[0], last = ctx->h_lon[ctx->nx - 1];
    if (!ctx->told_shortcuts_off && std::fabs(last - first - 360.0) < 0.01
        && !weights_stay_inside(ctx->coord_type, first, last)) {
      ctx->told_shortcuts_off = true;
      fprintf(stderr, "mptrac_hip: longitude axis %.17g ... %.17g does not span 360 degrees from a start in [-360, 0]: "
              "the early exits of deposition, convection and turbulent diffusion are off (mphip_get_shortcuts)\n", first, last);
    }
  }
  if (pk && reserve(ctx, ctx->codes[0], packed_block_bytes(pk)))
    return 1;
  if (upload_fields(ctx, S, met, new_grid, ctx->stream, pk, ctx->codes[0].p))
    return 1;
  HIPCHK(hipStreamSynchronize(ctx->stream));   // the host arrays may be reused by the caller
  S.time = met->time;
  S.valid = true;
  ctx->packed_dirty = true;
  return 0;
}

int mphip_update_met(mphip_ctx *ctx, int slot, const mphip_met_t *met) {
  return update_met_any(ctx, slot, met, nullptr);
}

int mphip_update_met_packed(mphip_ctx *ctx, int slot, const mphip_met_packed_t *met) {
  return update_met_any(ctx, slot, met ? &met->base : nullptr, met);
}

int mphip_swap_met(mphip_ctx *ctx) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  if (flush_meteo(ctx))
    return 1;
  ctx->flip ^= 1;
  ctx->packed_dirty = true;
  return 0;
}

// Page-lock the caller's particle arrays (option pin_host_atm) with ONE registration spanning all of them:
// a copy must lie inside a single registration, and neighbouring arrays of one allocation share pages, so
// per-array registrations are not an option.  Only done when the arrays lie close together (the members of
// an atm_t); failure is not an error -- the copies then go through the runtime's staging buffers.
static void pin_host_span(mphip_ctx *ctx, const void *const *ptrs, int n, size_t bytes_each) {
  if (!ctx->pin_host_atm || !bytes_each)
    return;
  uintptr_t lo = ~(uintptr_t) 0, hi = 0;
  size_t total = 0;
  for (int k = 0; k < n; k++)
    if (ptrs[k]) {
      lo = std::min(lo, (uintptr_t) ptrs[k]);
      hi = std::max(hi, (uintptr_t) ptrs[k] + bytes_each);
      total += bytes_each;
    }
  if (!total || hi - lo > total + total / 2 + (1u << 20))
    return;   // scattered arrays
  std::lock_guard<std::mutex> guard(ctx->pinned_lock);
  for (auto &r : ctx->pinned)
    if (lo >= r.first && hi <= r.second)
      return;
    else if (lo < r.second && hi > r.first)
      return;   // partly covered by an earlier span: leave it alone
  if (hipHostRegister((void *) lo, hi - lo, hipHostRegisterDefault) == hipSuccess)
    ctx->pinned.emplace_back(lo, hi);
  else
    (void) hipGetLastError();
}

// mphip_prefetch_met, and mphip_prefetch_met_packed (pk: the description `met` is the base of)
static int prefetch_met_any(mphip_ctx *ctx, const mphip_met_t *met, const mphip_met_packed_t *pk) {
  if (!ctx || !met)
    return fail(ctx, "bad argument");
  std::string why;
  if (pk && packed_refusal(pk, why))
    return fail(ctx, "mphip_prefetch_met_packed: " + why);
  HIPCHK(hipSetDevice(ctx->device));
  const int nml = met->npl > 0 ? met->npl : 0;
  if (!ctx->slot[0].valid || !ctx->slot[1].valid)
    return fail(ctx, "mphip_prefetch_met needs both snapshots on the device (mphip_update_met first)");
  if (met->nx != ctx->nx || met->ny != ctx->ny || met->np != ctx->npl || nml != ctx->nml)
    return fail(ctx, "Meteo grid dimensions do not match!");   // mptrac.c:6543-6546
  if (ctx->next_pending)
    return fail(ctx, "a prefetched snapshot is waiting for mphip_commit_met");
  if (!ctx->copy_stream) {
    HIPCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->next_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->main_mark, hipEventDisableTiming));
  }
  // the staging arrays of `next` were met0 until the last commit: kernels queued before it may still read them
  HIPCHK(hipEventRecord(ctx->main_mark, ctx->stream));
  HIPCHK(hipStreamWaitEvent(ctx->copy_stream, ctx->main_mark, 0));
  // Copies from ordinary (pageable) host memory keep the calling thread busy until they are done, and
  // page-locking arrays the caller owns is fragile (a copy has to lie inside one registration, arrays of
  // one allocation share pages, the caller may free them): an uploader thread of the library issues them
  // instead.  mphip_commit_met / mphip_discard_prefetch join it.
  if (pk && reserve(ctx, ctx->codes[1], packed_block_bytes(pk)))
    return 1;
  // (the uploader thread reads its own copy of the description: its base, and the packed one when there is one)
  mphip_met_packed_t desc_pk;
  memset(&desc_pk, 0, sizeof(desc_pk));
  if (pk)
    desc_pk = *pk;
  else
    desc_pk.base = *met;
  const bool coded = pk != nullptr;
  ctx->uploader_rc = 0;
  ctx->uploader_done = false;
  ctx->uploader_err.clear();
  ctx->next_pending = true;
  ctx->next.time = met->time;
  ctx->next.lon.assign(met->lon, met->lon + met->nx);
  ctx->next.lat.assign(met->lat, met->lat + met->ny);
  ctx->next.p.assign(met->p, met->p + met->np);
  // The packed grids of the step after the hand-over -- (today's met1, the new snapshot) -- are built on the copy
  // stream as well, into the second set of packed arrays: the hand-over then costs the stepping stream nothing.
  // Which fields the new snapshot carries is known from its description; the arrays are allocated here, on the
  // calling thread, the uploader thread only launches.  (Pressure-level configurations; the model-level records
  // depend on a monotonicity check that is read back, and on ADVECT_VERT_COORD: they are packed at the commit.)
  ctx->pk_next_valid = false;
  bool pack_ahead = ctx->nml == 0;
  PackPlan plan;
  if (pack_ahead) {
    MetSlot probe;   // (presence flags only)
    for (int f = 0; f < MPHIP_N3D; f++)
      probe.has3[f] = met->f3[f] != nullptr || (pk && pk->q3[f]);
    for (int f = 0; f < MPHIP_N2D; f++)
      probe.has2[f] = met->f2[f] != nullptr;
    plan = pack_plan(ctx, ctx->slot[1 ^ ctx->flip], probe);
    if (pack_alloc(ctx, ctx->pk_next, plan))
      return 1;
  }
  ctx->uploader = std::thread([ctx, desc_pk, coded, pack_ahead, plan]() {
    int rc = hipSetDevice(ctx->device) == hipSuccess ? 0 : 1;
    if (!rc)   // (a packed field: its copy, then its decode, on the copy stream)
      rc = upload_fields(ctx, ctx->next, &desc_pk.base, false, ctx->copy_stream, coded ? &desc_pk : nullptr, ctx->codes[1].p);
    if (!rc && pack_ahead) {
      // met1 of today is met0 after the commit; its staging arrays are not written while it is a current slot
      rc = pack_launch(ctx, ctx->pk_next, plan, ctx->slot[1 ^ ctx->flip], ctx->next, ctx->copy_stream);
      ctx->pk_next_valid = rc == 0;
    }
    if (!rc && hipEventRecord(ctx->next_ready, ctx->copy_stream) != hipSuccess)
      rc = 1;
    ctx->uploader_rc = rc;
    ctx->uploader_done = true;
  });
  return 0;
}

int mphip_prefetch_met(mphip_ctx *ctx, const mphip_met_t *met) {
  return prefetch_met_any(ctx, met, nullptr);
}

int mphip_prefetch_met_packed(mphip_ctx *ctx, const mphip_met_packed_t *met) {
  return prefetch_met_any(ctx, met ? &met->base : nullptr, met);
}

int mphip_derive_met(mphip_ctx *ctx, const mphip_met_t *in, unsigned what, const mphip_prep_t *opt, const mphip_met_out_t *out) {
  if (!ctx || !in || !opt || !out)
    return fail(ctx, "mphip_derive_met: null argument");
  constexpr unsigned kAll = MPHIP_PREP_GEOPOT | MPHIP_PREP_O3C | MPHIP_PREP_PBL | MPHIP_PREP_CLOUD | MPHIP_PREP_CAPE
    | MPHIP_PREP_PV | MPHIP_PREP_TROPO;
  if (!what || (what & ~kAll))
    return fail(ctx, "mphip_derive_met: `what` must be an OR of MPHIP_PREP_* bits");
  if (const char *why = grid_refusal(in->nx, in->ny, in->np, in->lon && in->lat && in->p))
    return fail(ctx, std::string("mphip_derive_met: ") + why);
  if (!regrid_strides_ok(in->ny, in->np, in->sx, in->sy) || in->sx2 < in->ny)
    return fail(ctx, "mphip_derive_met: unsupported meteo strides");
  for (int k = 1; k < in->np; k++)
    if (!(in->p[k] < in->p[k - 1]))
      return fail(ctx, "mphip_derive_met: the pressure axis must be strictly descending");
  // inputs and outputs of the requested bits
  bool need3[MPHIP_N3D] = {}, need2[MPHIP_N2D] = {}, give2[MPHIP_N2D] = {};
  const bool geopot = what & MPHIP_PREP_GEOPOT;
  auto missing = [&](const char *bit, const char *names) {
    return fail(ctx, std::string("mphip_derive_met: ") + bit + " needs the fields " + names);
  };
  auto have3 = [&](std::initializer_list<int> f) {
    bool ok = true;
    for (int k : f) {
      ok = ok && in->f3[k];
      need3[k] = true;
    }
    return ok;
  };
  auto have2 = [&](std::initializer_list<int> f) {
    bool ok = true;
    for (int k : f) {
      ok = ok && in->f2[k];
      need2[k] = true;
    }
    return ok;
  };
  auto outputs = [&](std::initializer_list<int> f) {
    bool ok = true;
    for (int k : f) {
      ok = ok && out->f2[k];
      give2[k] = true;
    }
    return ok;
  };
  int sx = 0, sy = 0;
  if (geopot) {
    if (!(have3({ MPHIP_T, MPHIP_H2O }) & have2({ MPHIP_PS, MPHIP_ZS })))
      return missing("MPHIP_PREP_GEOPOT", "t, h2o, ps, zs");
    if (!out->f3[MPHIP_Z])
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_GEOPOT needs the output array z");
    sx = opt->met_geopot_sx;
    sy = opt->met_geopot_sy;
    if (sx < 0 || sy < 0) {
      const bool fine = fabs(in->lon[1] - in->lon[0]) < 0.5;
      sx = fine ? 3 : 6;
      sy = fine ? 2 : 4;
    }
    if (sx == 0 || sy == 0)
      sx = sy = 0;
    if (sx > 0 && (sx - 1 > in->nx
                   || (size_t) (kSmTX + 2 * (sx - 1)) * (kSmTY + 2 * (sy - 1)) * kSmKC * sizeof(float) > 64 * 1024))
      return fail(ctx, "mphip_derive_met: smoothing half-widths too large (met_geopot_sx - 1 <= nx, tile within 64 KB of LDS)");
  }
  if (what & MPHIP_PREP_O3C) {
    if (!(have3({ MPHIP_O3 }) & have2({ MPHIP_PS })))
      return missing("MPHIP_PREP_O3C", "o3, ps");
    if (!outputs({ MPHIP_O3C }))
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_O3C needs the output array o3c");
  }
  if (what & MPHIP_PREP_PBL) {
    if (opt->met_pbl != 2 && opt->met_pbl != 3)
      return fail(ctx, "mphip_derive_met: met_pbl must be 2 (bulk Richardson number) or 3 (potential temperature)");
    if (!(have3({ MPHIP_T }) & have2({ MPHIP_PS, MPHIP_TS })))
      return missing("MPHIP_PREP_PBL", "t, ps, ts");
    if (opt->met_pbl == 2) {
      if (!(have3({ MPHIP_U, MPHIP_V, MPHIP_H2O }) & have2({ MPHIP_US, MPHIP_VS, MPHIP_ZS })) || (!geopot && !in->f3[MPHIP_Z]))
        return missing("MPHIP_PREP_PBL with met_pbl 2", "t, h2o, u, v, ps, ts, us, vs, zs and z (given, or MPHIP_PREP_GEOPOT in the same call)");
      if (!geopot)
        need3[MPHIP_Z] = true;
    }
    if (!outputs({ MPHIP_PBL }))
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_PBL needs the output array pbl");
  }
  if (what & MPHIP_PREP_CLOUD) {
    if (!(have3({ MPHIP_LWC, MPHIP_IWC }) & have2({ MPHIP_PS })))
      return missing("MPHIP_PREP_CLOUD", "lwc, iwc, ps");
    need3[MPHIP_RWC] = in->f3[MPHIP_RWC] != nullptr;
    need3[MPHIP_SWC] = in->f3[MPHIP_SWC] != nullptr;
    if (!outputs({ MPHIP_PCT, MPHIP_PCB, MPHIP_CL }))
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_CLOUD needs the output arrays pct, pcb, cl");
  }
  if (what & MPHIP_PREP_CAPE) {
    if (!(have3({ MPHIP_T, MPHIP_H2O }) & have2({ MPHIP_PS })))
      return missing("MPHIP_PREP_CAPE", "t, h2o, ps");
    if (!ctx->have_clim)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_CAPE needs the tropopause climatology (mphip_update_clim first)");
    if (in->coord_type != 0 && !ctx->have_ctl)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_CAPE on a Cartesian grid needs met_utm_ref_lat (mphip_update_ctl first)");
    if (!outputs({ MPHIP_PLCL, MPHIP_PLFC, MPHIP_PEL, MPHIP_CAPE, MPHIP_CIN }))
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_CAPE needs the output arrays plcl, plfc, pel, cape, cin");
  }
  const bool do_pv = what & MPHIP_PREP_PV, tropo = what & MPHIP_PREP_TROPO;
  if (do_pv) {
    if (!have3({ MPHIP_T, MPHIP_U, MPHIP_V }))
      return missing("MPHIP_PREP_PV", "t, u, v");
    if (!out->f3[MPHIP_PV])
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_PV needs the output array pv");
    if (in->coord_type != 0)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_PV needs a longitude / latitude grid (coord_type 0)");
    if (in->ny < 5)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_PV needs two columns and five rows or more (nx < 2 or ny < 5)");
  }
  size_t lds_tropo = 0;
  int c_tropo = 0, tropo_nprof = 0, tropo_fine = 0;
  if (tropo) {
    const int mode = opt->met_tropo;
    if (mode < 1 || mode > 5)
      return fail(ctx, "mphip_derive_met: met_tropo must be 1 (climatology), 2 (cold point), 3 (WMO first), 4 (WMO second) "
                  "or 5 (dynamical)");
    if (opt->met_tropo_spline != 0 && opt->met_tropo_spline != 1)
      return fail(ctx, "mphip_derive_met: met_tropo_spline must be 0 (linear) or 1 (cubic)");
    if (mode != 1 && in->np < 3)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_TROPO with met_tropo 2 to 5 needs three pressure levels or more "
                  "(np < 3)");
    if (!have3({ MPHIP_T, MPHIP_H2O }) || (!geopot && !in->f3[MPHIP_Z]))
      return missing("MPHIP_PREP_TROPO", "t, h2o and z (given, or MPHIP_PREP_GEOPOT in the same call)");
    if (!geopot)
      need3[MPHIP_Z] = true;
    if (mode == 5) {
      if (!do_pv && !in->f3[MPHIP_PV])
        return missing("MPHIP_PREP_TROPO with met_tropo 5", "pv (given, or MPHIP_PREP_PV in the same call)");
      if (!do_pv)
        need3[MPHIP_PV] = true;
    }
    if (mode == 1 && !ctx->have_clim)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_TROPO with met_tropo 1 needs the tropopause climatology "
                  "(mphip_update_clim first)");
    if (mode == 1 && in->coord_type != 0 && !ctx->have_ctl)
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_TROPO with met_tropo 1 on a Cartesian grid needs met_utm_ref_lat "
                  "(mphip_update_ctl first)");
    if (!outputs({ MPHIP_PT, MPHIP_TT, MPHIP_ZT, MPHIP_H2OT }))
      return fail(ctx, "mphip_derive_met: MPHIP_PREP_TROPO needs the output arrays pt, tt, zt, h2ot");
    // the axis tables, per column c[np] and (met_tropo 3, 4) the fine profile in double, and the staged profiles (t; t and
    // pv with met_tropo 5)
    tropo_nprof = mode == 1 ? 0 : (mode == 5 ? 2 : 1);
    tropo_fine = mode == 3 || mode == 4 ? kTropoFine : 0;
    c_tropo = columns_per_workgroup(
      [&](int cpb) {
        return ((size_t) 6 * in->np + 2 * kTropoFine + (size_t) cpb * (in->np + tropo_fine)) * sizeof(double)
          + (size_t) tropo_nprof * cpb * (in->np | 1) * sizeof(float);
      },
      &lds_tropo);
  }
  const int np = in->np;
  // a column kernel that stages nf fields
  auto columns = [np](int nf, size_t *lds) {
    return columns_per_workgroup(
      [=](int cpb) { return 2 * (size_t) np * sizeof(double) + (size_t) nf * cpb * (np | 1) * sizeof(float); }, lds);
  };
  size_t lds_geo = 0, lds_o3 = 0, lds_cloud = 0, lds_pbl = 0, lds_cape = 0;
  const int c_geo = columns(3, &lds_geo), c_o3 = columns(1, &lds_o3), c_cloud = columns(4, &lds_cloud);
  const int c_pbl = columns(opt->met_pbl == 2 ? 5 : 1, &lds_pbl), c_cape = columns(2, &lds_cape);
  if ((geopot && !c_geo) || ((what & MPHIP_PREP_O3C) && !c_o3) || ((what & MPHIP_PREP_CLOUD) && !c_cloud)
      || ((what & MPHIP_PREP_PBL) && !c_pbl) || ((what & MPHIP_PREP_CAPE) && !c_cape) || (tropo && !c_tropo))
    return fail(ctx, "mphip_derive_met: too many pressure levels for one column in 64 KB of LDS");

  std::vector<double> tab;      // (declared before the call scope: it outlives the scope's last synchronisation)
  PrepCall call(ctx);
  if (call.open())
    return 1;
  hipStream_t st = call.st;
  const int nx = in->nx, ny = in->ny;
  const size_t ncol = (size_t) nx * ny, ncell = ncol * np;
  if (call.mark_begin(1))
    return 1;
  // p[np] | lat[ny] | lon[nx] | the tropopause's tables (PrepTropo::tab)
  double *const d_p = call.take<double>((size_t) np + ny + nx + 5 * (size_t) np + 2 * kTropoFine);
  if (!d_p)
    return 1;
  double *const d_lat = d_p + np, *const d_lon = d_lat + ny, *const d_tab = d_lon + nx;
  HIPCHK(hipMemcpyAsync(d_p, in->p, (size_t) np * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_lat, in->lat, (size_t) ny * sizeof(double), hipMemcpyHostToDevice, st));
  if (do_pv || tropo) {
    // what depends on the pressure axis alone, with the host's C library -- the one mphip_libm.h restates, so these are
    // the values the device functions would give --: pows = pow(1000 / p, 0.286) and, for met_tropo 2 ... 5 only, zc =
    // Z(p), the spline's interval widths h, elimination factors w and eliminated diagonal d, z2 and p2 = P(z2).  The
    // recurrence of d must keep its two roundings (the definition's `d[i] -= w o[i-1]`): the product is rounded on its
    // own line, whatever the host compiler may contract.
    tab.assign(5 * (size_t) np + 2 * kTropoFine, 0.0);
    double *zc = tab.data(), *h = zc + np, *w = h + np, *d = w + np, *pows = d + np, *z2 = pows + np, *p2 = z2 + kTropoFine;
    for (int k = 0; k < np; k++)
      pows[k] = pow(1000. / in->p[k], 0.286);
    if (tropo && opt->met_tropo != 1) {
      for (int k = 0; k < np; k++)
        zc[k] = 7 * log(1013.25 / in->p[k]);
      for (int k = 0; k + 1 < np; k++)
        h[k] = zc[k + 1] - zc[k];
      for (int i = 0; i + 3 <= np; i++) {
        d[i] = 2 * (h[i] + h[i + 1]);
        if (i > 0) {
          w[i] = h[i] / d[i - 1];
          volatile double wh = w[i] * h[i];
          d[i] -= wh;
        }
      }
      for (int i = 0; i < kTropoFine; i++) {
        z2[i] = 4.5 + 0.1 * i;
        p2[i] = 1013.25 * exp(-z2[i] / 7.);
      }
    }
    HIPCHK(hipMemcpyAsync(d_lon, in->lon, (size_t) nx * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  float *i3[MPHIP_N3D] = {}, *i2[MPHIP_N2D] = {}, *o2[MPHIP_N2D] = {};
  const LevelField L = { np, in->sx, in->sy };
  for (int f = 0; f < MPHIP_N3D; f++)
    if (need3[f] && !(i3[f] = call.upload3(in->f3[f], nx, ny, L)))
      return 1;
  for (int f = 0; f < MPHIP_N2D; f++) {
    if (need2[f] && !(i2[f] = call.upload2(in->f2[f], nx, ny, in->sx2)))
      return 1;
    if (give2[f] && !(o2[f] = call.take<float>(ncol)))
      return 1;
  }
  // geopotential height before and after the smoothing; potential vorticity
  float *z_raw = nullptr, *z_smooth = nullptr, *pv = nullptr;
  if (geopot && (!(z_raw = call.take<float>(ncell)) || (sx > 0 && !(z_smooth = call.take<float>(ncell)))))
    return 1;
  if (do_pv && !(pv = call.take<float>(ncell)))
    return 1;
  if (call.mark_end())
    return 1;

  PrepGrid G;
  G.nx = nx;
  G.ny = ny;
  G.np = np;
  G.pitch = np | 1;
  G.ncol = (int) ncol;
  G.p = d_p;
  G.lat = d_lat;
  PrepOpt O;
  O.met_pbl = opt->met_pbl;
  O.pbl_min = opt->met_pbl_min;
  O.pbl_max = opt->met_pbl_max;
  O.cloud_min = opt->met_cloud_min;
  O.time = in->time;
  O.coord_type = in->coord_type;
  O.ref_lat = ctx->have_ctl ? ctx->ctl.met_utm_ref_lat : 0.0;
  const dim3 lanes(kPrepLanes);
  auto blocks = [&](int cpb) {
    G.cpb = cpb;
    return dim3((unsigned) ((ncol + cpb - 1) / cpb));
  };
  float *z_final = i3[MPHIP_Z];
  if (geopot) {
    const dim3 nb = blocks(c_geo);
    if (call.launch(prep_geopot_kernel, nb, lanes, lds_geo, G, i3[MPHIP_T], i3[MPHIP_H2O], i2[MPHIP_PS], i2[MPHIP_ZS], z_raw))
      return 1;
    z_final = z_raw;
    if (sx > 0) {
      const size_t lds = (size_t) (kSmTX + 2 * (sx - 1)) * (kSmTY + 2 * (sy - 1)) * kSmKC * sizeof(float);
      const dim3 tiles((nx + kSmTX - 1) / kSmTX, (ny + kSmTY - 1) / kSmTY, (np + kSmKC - 1) / kSmKC);
      if (call.launch(prep_smooth_kernel, tiles, dim3(256), lds, G, sx, sy, z_raw, z_smooth))
        return 1;
      z_final = z_smooth;
    }
  }
  if (what & MPHIP_PREP_O3C) {
    const dim3 nb = blocks(c_o3);
    if (call.launch(prep_o3c_kernel, nb, lanes, lds_o3, G, i3[MPHIP_O3], i2[MPHIP_PS], o2[MPHIP_O3C]))
      return 1;
  }
  if (what & MPHIP_PREP_CLOUD) {
    const dim3 nb = blocks(c_cloud);
    if (call.launch(prep_cloud_kernel, nb, lanes, lds_cloud, G, O, i3[MPHIP_LWC], i3[MPHIP_RWC], i3[MPHIP_IWC], i3[MPHIP_SWC],
                    i2[MPHIP_PS], o2[MPHIP_PCT], o2[MPHIP_PCB], o2[MPHIP_CL]))
      return 1;
  }
  if (what & MPHIP_PREP_PBL) {
    const dim3 nb = blocks(c_pbl);
    const bool ri = opt->met_pbl == 2;
    if (call.launch(prep_pbl_kernel, nb, lanes, lds_pbl, G, O, i3[MPHIP_T], ri ? i3[MPHIP_H2O] : nullptr,
                    ri ? i3[MPHIP_U] : nullptr, ri ? i3[MPHIP_V] : nullptr, ri ? z_final : nullptr, i2[MPHIP_PS], i2[MPHIP_TS],
                    ri ? i2[MPHIP_ZS] : nullptr, ri ? i2[MPHIP_US] : nullptr, ri ? i2[MPHIP_VS] : nullptr, o2[MPHIP_PBL]))
      return 1;
  }
  if (what & MPHIP_PREP_CAPE) {
    const dim3 nb = blocks(c_cape);
    if (call.launch(prep_cape_kernel, nb, lanes, lds_cape, G, O, ctx->d_clim.p, i3[MPHIP_T], i3[MPHIP_H2O], i2[MPHIP_PS],
                    o2[MPHIP_PLCL], o2[MPHIP_PLFC], o2[MPHIP_PEL], o2[MPHIP_CAPE], o2[MPHIP_CIN]))
      return 1;
  }
  float *pv_final = i3[MPHIP_PV];
  if (do_pv) {
    // (the field and its polar rows: one event pair)
    const dim3 tiles((nx + kPvTX - 1) / kPvTX, (ny + kPvTY - 1) / kPvTY, (np + kPvKC - 1) / kPvKC);
    if (call.mark_begin(0)
        || call.enqueue(prep_pv_kernel, tiles, dim3(256), kPvLds, G, d_lon, d_tab + 4 * (size_t) np, i3[MPHIP_T], i3[MPHIP_U],
                        i3[MPHIP_V], pv)
        || call.enqueue(prep_pv_polar_kernel, dim3((unsigned) (((size_t) nx * np + 255) / 256)), dim3(256), 0, G, pv)
        || call.mark_end())
      return 1;
    pv_final = pv;
  }
  if (tropo) {
    const dim3 nb = blocks(c_tropo);
    PrepTropo T;
    T.mode = opt->met_tropo;
    T.spline = opt->met_tropo_spline;
    T.pv_thr = opt->met_tropo_pv;
    T.theta_thr = opt->met_tropo_theta;
    T.nprof = tropo_nprof;
    T.fine = tropo_fine;
    T.tab = d_tab;
    if (call.launch(prep_tropo_kernel, nb, lanes, lds_tropo, G, O, T, ctx->d_clim.p, i3[MPHIP_T], i3[MPHIP_H2O], z_final,
                    T.mode == 5 ? pv_final : nullptr, o2[MPHIP_PT], o2[MPHIP_TT], o2[MPHIP_ZT], o2[MPHIP_H2OT]))
      return 1;
  }
  if (call.mark_begin(2))
    return 1;
  if (do_pv && call.download3(pv, out->f3[MPHIP_PV], nx, ny, L))
    return 1;
  if (geopot && call.download3(z_final, out->f3[MPHIP_Z], nx, ny, L))
    return 1;
  for (int f = 0; f < MPHIP_N2D; f++)
    if (give2[f] && call.download2(o2[f], out->f2[f], nx, ny, in->sx2))
      return 1;
  return call.close();
}

size_t mphip_sizeof_regrid(void) {
  return sizeof(mphip_regrid_t);
}

int mphip_regrid_shape(const mphip_met_t *in, unsigned what, const mphip_regrid_t *opt, int *nx2, int *ny2, int *np2) {
  if (!in || !opt)
    return 1;
  RegridPlan P;
  if (regrid_plan(in, what, opt, &P))
    return 1;
  if (nx2)
    *nx2 = P.nx2;
  if (ny2)
    *ny2 = P.ny2;
  if (np2)
    *np2 = P.np2;
  return 0;
}

int mphip_regrid_met(mphip_ctx *ctx, const mphip_met_t *in, unsigned what, const mphip_regrid_t *opt,
                     const mphip_regrid_out_t *out) {
  if (!ctx || !in || !opt || !out)
    return fail(ctx, "mphip_regrid_met: null argument");
  RegridPlan P;
  if (const char *why = regrid_plan(in, what, opt, &P))
    return fail(ctx, std::string("mphip_regrid_met: ") + why);
  const bool ml = what & MPHIP_REGRID_ML2PL, sample = what & MPHIP_REGRID_SAMPLE;
  if (!in->lon || !in->lat || (!ml && !in->p))
    return fail(ctx, "mphip_regrid_met: the input axes are missing");
  if (ml && !in->f3[MPHIP_PL])
    return fail(ctx, "mphip_regrid_met: MPHIP_REGRID_ML2PL needs the field pl");
  if (!regrid_strides_ok(P.ny, P.np0, in->sx, in->sy) || in->sx2 < P.ny
      || (ml && !regrid_strides_ok(P.ny, P.np0, in->sx_ml, in->sy_ml)))
    return fail(ctx, "mphip_regrid_met: unsupported meteo strides");
  if (!regrid_strides_ok(P.ny2, P.np2, out->sx, out->sy) || out->sx2 < P.ny2)
    return fail(ctx, "mphip_regrid_met: the output strides do not hold the output grid");
  // the fields of this call: present on both sides
  int f3[kRgFields + 2], n3 = 0, f2[MPHIP_N2D], n2 = 0;
  for (int i = 0; i < (ml ? kRgFields : kRgFields + 2); i++) {
    const int f = ml ? kRegridMl[i] : kRegridPl[i];
    if (in->f3[f] && out->f3[f])
      f3[n3++] = f;
  }
  for (int f = 0; f < MPHIP_N2D; f++)
    if (in->f2[f] && out->f2[f])
      f2[n2++] = f;

  PrepCall call(ctx);
  if (call.open())
    return 1;
  hipStream_t st = call.st;
  const size_t ncol = (size_t) P.nx * P.ny, ncol2 = (size_t) P.nx2 * P.ny2;
  const size_t ncell1 = ncol * P.np1, ncell2 = ncol2 * P.np2;
  // the axes of the output are taken before anything is written (`out` may alias `in`)
  std::vector<double> lon2(P.nx2), lat2(P.ny2), p2(P.np2);
  const int ddx = sample ? opt->met_dx : 1, ddy = sample ? opt->met_dy : 1, ddp = sample ? opt->met_dp : 1;
  for (int i = 0; i < P.nx2; i++)
    lon2[i] = in->lon[(size_t) i * ddx];
  for (int i = 0; i < P.ny2; i++)
    lat2[i] = in->lat[(size_t) i * ddy];
  for (int i = 0; i < P.np2; i++)
    p2[i] = (ml ? opt->met_p : in->p)[(size_t) i * ddp];

  // uploads; per field of the call the uploaded array, ML2PL's result and SAMPLE's result
  float *in3[kRgFields + 2] = {}, *mid3[kRgFields + 2] = {}, *out3[kRgFields + 2] = {}, *in2[MPHIP_N2D] = {}, *out2[MPHIP_N2D] = {};
  double *d_metp = nullptr;
  float *d_pl = nullptr;
  if (call.mark_begin(1))
    return 1;
  if (ml) {
    if (!(d_metp = call.take<double>((size_t) opt->met_np)))
      return 1;
    HIPCHK(hipMemcpyAsync(d_metp, opt->met_p, (size_t) opt->met_np * sizeof(double), hipMemcpyHostToDevice, st));
    if (!(d_pl = call.upload3(in->f3[MPHIP_PL], P.nx, P.ny, LevelField{ P.np0, in->sx_ml, in->sy_ml })))
      return 1;
  }
  for (int i = 0; i < n3; i++) {
    if (!(in3[i] = call.upload3(in->f3[f3[i]], P.nx, P.ny, LevelField{ P.np0, in->sx, in->sy })))
      return 1;
    if (ml && !(mid3[i] = call.take<float>(ncell1)))
      return 1;
    if (sample && !(out3[i] = call.take<float>(ncell2)))
      return 1;
  }
  for (int i = 0; i < n2; i++) {
    if (!(in2[i] = call.upload2(in->f2[f2[i]], P.nx, P.ny, in->sx2)))
      return 1;
    if (sample && !(out2[i] = call.take<float>(ncol2)))
      return 1;
  }
  if (call.mark_end() || call.uploads_complete())
    return 1;

  if (ml && n3 > 0) {
    RegridFields F;
    F.n = n3;
    for (int i = 0; i < n3; i++) {
      F.in[i] = in3[i];
      F.out[i] = mid3[i];
    }
    if (call.launch(regrid_ml2pl_kernel, dim3((unsigned) ((ncol + P.ml_cpb - 1) / P.ml_cpb)), dim3(kRgThreads), P.ml_lds,
                    (int) ncol, P.np0, opt->met_np, P.ml_cpb, P.np0 | 1, d_metp, d_pl, F))
      return 1;
  }
  if (sample) {
    const dim3 tiles3((P.nx2 + kRgTX - 1) / kRgTX, (P.ny2 + kRgTY - 1) / kRgTY, (P.np2 + kRgKC - 1) / kRgKC);
    const dim3 tiles2(tiles3.x, tiles3.y, 1);
    for (int i = 0; i < n3; i++)
      if (call.launch(regrid_sample_kernel<kRgKC>, tiles3, dim3(kRgThreads), P.lds3, P.S3, ml ? mid3[i] : in3[i], out3[i]))
        return 1;
    for (int i = 0; i < n2; i++)
      if (call.launch(regrid_sample_kernel<1>, tiles2, dim3(kRgTX * kRgTY), P.lds2, P.S2, in2[i], out2[i]))
        return 1;
  }
  if (call.mark_begin(2))
    return 1;
  for (int i = 0; i < n3; i++)
    if (call.download3(sample ? out3[i] : mid3[i], out->f3[f3[i]], P.nx2, P.ny2, LevelField{ P.np2, out->sx, out->sy }))
      return 1;
  for (int i = 0; i < n2; i++)
    if (call.download2(sample ? out2[i] : in2[i], out->f2[f2[i]], P.nx2, P.ny2, out->sx2))
      return 1;
  if (call.close())
    return 1;
  call.write_axes(out, lon2, lat2, p2);
  return 0;
}

size_t mphip_sizeof_detrend(void) {
  return sizeof(mphip_detrend_t);
}

int mphip_detrend_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_detrend_t *opt, const mphip_regrid_out_t *out) {
  if (!ctx || !in || !opt || !out)
    return fail(ctx, "mphip_detrend_met: null argument");
  if (!in->lon || !in->lat || !in->p)
    return fail(ctx, "mphip_detrend_met: the input axes are missing");
  DetrendPlan P;
  if (const char *why = detrend_plan(in, opt, &P))
    return fail(ctx, std::string("mphip_detrend_met: ") + why);
  if (!regrid_strides_ok(P.ny, P.np, in->sx, in->sy))
    return fail(ctx, "mphip_detrend_met: unsupported meteo strides");
  if (!regrid_strides_ok(P.ny, P.np, out->sx, out->sy))
    return fail(ctx, "mphip_detrend_met: the output strides do not hold the grid");
  int fld[kDtFields], nf = 0;
  for (int i = 0; i < kDtFields; i++)
    if (in->f3[kDetrendFields[i]] && out->f3[kDetrendFields[i]])
      fld[nf++] = kDetrendFields[i];
  if (!nf)
    return fail(ctx, "mphip_detrend_met: none of the fields t, u, v, w is present in both `in` and `out`");

  std::vector<float> w;         // (as P.rows, declared before the call scope: it outlives the scope's last synchronisation)
  PrepCall call(ctx);
  if (call.open())
    return 1;
  hipStream_t st = call.st;
  // the weight table (host; the stream is idle meanwhile, so the two events around it give the host's time)
  if (call.mark_begin(3))
    return 1;
  detrend_table(in, P, w);
  if (call.mark_end())
    return 1;
  // uploads
  if (call.mark_begin(1))
    return 1;
  const size_t ncell = (size_t) P.nx * P.ny * P.np;
  float *const d_w = call.take<float>(P.nw);
  DetrendRow *const d_rows = d_w ? call.take<DetrendRow>((size_t) P.ny) : nullptr;
  if (!d_rows)
    return 1;
  HIPCHK(hipMemcpyAsync(d_w, w.data(), P.nw * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_rows, P.rows.data(), (size_t) P.ny * sizeof(DetrendRow), hipMemcpyHostToDevice, st));
  DetrendFields F;
  memset(&F, 0, sizeof(F));
  F.n = nf;
  float *res[kDtFields] = {};
  for (int i = 0; i < nf; i++) {
    float *const d_in = call.take<float>(ncell);
    if (!d_in || !(res[i] = call.take<float>(ncell))
        || call.to_device3(d_in, in->f3[fld[i]], P.nx, P.ny, LevelField{ P.np, in->sx, in->sy }))
      return 1;
    F.in[i] = d_in;
    F.out[i] = res[i];
  }
  if (call.mark_end() || call.uploads_complete())     // (the table and the row records are this call's own vectors)
    return 1;

  if (call.launch(detrend_kernel, dim3((unsigned) ((long long) P.nchunk * P.ny), (unsigned) nf), dim3(kDtThreads), 0, P.nx, P.ny,
                  P.np, d_rows, d_w, F))
    return 1;
  if (call.mark_begin(2))
    return 1;
  for (int i = 0; i < nf; i++)
    if (call.download3(res[i], out->f3[fld[i]], P.nx, P.ny, LevelField{ P.np, out->sx, out->sy }))
      return 1;
  return call.close();
}

// ---- mphip_ingest_met (mphip_ingest.hpp) -------------------------------------------------------------------------------
size_t mphip_sizeof_ingest_raw(void) {
  return sizeof(mphip_ingest_raw_t);
}

// what mphip_ingest_shape and mphip_ingest_met refuse of the grid and of `what`, and which of POLAR and PERIODIC act;
// NULL = accepted
struct IngestPlan {
  int nx, ny, np, nx2;
  bool polar, periodic;
};

static const char *ingest_plan(const mphip_met_t *in, unsigned what, IngestPlan *P) {
  const unsigned all = MPHIP_INGEST_DECODE | MPHIP_INGEST_EXTRAPOLATE | MPHIP_INGEST_POLAR | MPHIP_INGEST_PERIODIC;
  if (!what || (what & ~all))
    return "`what` must be an OR of MPHIP_INGEST_* bits";
  if (!in->lon || !in->lat || !in->p)
    return "the input axes are missing";
  if (const char *why = grid_refusal(in->nx, in->ny, in->np))
    return why;
  if (const char *why = grid_size_refusal(in->nx, in->ny, std::max(in->np, in->npl)))
    return why;
  P->nx = in->nx;
  P->ny = in->ny;
  P->np = in->np;
  const double *lon = in->lon, *lat = in->lat;
  P->polar = (what & MPHIP_INGEST_POLAR) && in->coord_type == 0 && fabs(lat[0]) >= 89.999 && fabs(lat[in->ny - 1]) >= 89.999;
  P->periodic = (what & MPHIP_INGEST_PERIODIC) && in->coord_type == 0
    && fabs(lon[in->nx - 1] - lon[0] + lon[1] - lon[0] - 360) < 0.01;
  P->nx2 = in->nx + (P->periodic ? 1 : 0);
  return grid_size_refusal(P->nx2, in->ny, std::max(in->np, in->npl));
}

int mphip_ingest_shape(const mphip_met_t *in, unsigned what, int *nx2) {
  IngestPlan P;
  if (!in || !nx2 || ingest_plan(in, what, &P))
    return 1;
  *nx2 = P.nx2;
  return 0;
}

int mphip_ingest_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_ingest_raw_t *raw, unsigned what,
                     const mphip_regrid_out_t *out) {
  const bool decode = what & MPHIP_INGEST_DECODE;
  if (!ctx || !in || !out || (decode && !raw))
    return fail(ctx, "mphip_ingest_met: null argument");
  IngestPlan P;
  if (const char *why = ingest_plan(in, what, &P))
    return fail(ctx, std::string("mphip_ingest_met: ") + why);
  // the fields of this call: given raw or in met order, and named in `out`
  struct Field {
    bool is3;
    int f, nlev;
    const mphip_raw_t *raw;     // NULL: in met order
    const float *src;
    float *dst, *dev;
    LevelField L;               // of src (3-D)
  } fld[MPHIP_N3D + MPHIP_N2D];
  int nf = 0;
  for (int i = 0; i < MPHIP_N3D + MPHIP_N2D; i++) {
    const bool is3 = i < MPHIP_N3D;
    const int f = is3 ? i : i - MPHIP_N3D;
    const char *name = is3 ? kField3Name[f] : kField2Name[f];
    const mphip_raw_t *r = decode ? (is3 ? &raw->f3[f] : &raw->f2[f]) : nullptr;
    const float *src = is3 ? in->f3[f] : in->f2[f];
    float *dst = is3 ? out->f3[f] : out->f2[f];
    if (r && r->type == 0)
      r = nullptr;
    if (r) {
      if (r->type != MPHIP_RAW_FLOAT && r->type != MPHIP_RAW_SHORT)
        return fail(ctx, std::string("mphip_ingest_met: field ") + name + " has a raw descriptor of unknown type");
      if (src)
        return fail(ctx, std::string("mphip_ingest_met: field ") + name + " is given both raw and in met order");
      if (r->lnsp && (is3 || f != MPHIP_PS))
        return fail(ctx, std::string("mphip_ingest_met: field ") + name + ": lnsp belongs to the surface pressure alone");
      if (dst && !r->data)
        return fail(ctx, std::string("mphip_ingest_met: field ") + name + " has a raw descriptor without data");
    }
    if ((!r && !src) || !dst)
      continue;
    if (is3 && field_on_model_levels(f) && in->npl < 1)
      return fail(ctx, std::string("mphip_ingest_met: field ") + name + " is on model levels and npl < 1");
    const LevelField L = is3 ? level_field(in, f) : LevelField{ 1, 0, 0 };
    if (!r && (is3 ? !regrid_strides_ok(P.ny, L.nlev, L.sx, L.sy) : in->sx2 < P.ny))
      return fail(ctx, "mphip_ingest_met: unsupported meteo strides");
    if (is3 ? !regrid_strides_ok(P.ny, L.nlev, out->sx, out->sy) : out->sx2 < P.ny)
      return fail(ctx, "mphip_ingest_met: the output strides do not hold the grid");
    fld[nf++] = Field{ is3, f, L.nlev, r, src, dst, nullptr, L };
  }
  if (!nf)
    return fail(ctx, "mphip_ingest_met: no field is given in `in` or `raw` and named in `out`");

  // the axes of the output and the frames of the two poles are taken before anything is written (`out` may alias `in`)
  const int nx = P.nx, ny = P.ny, np = P.np, nx2 = P.nx2;
  std::vector<double> lon2(in->lon, in->lon + nx), lat2(in->lat, in->lat + ny), p2(in->p, in->p + np);
  if (P.periodic)
    lon2.push_back(in->lon[nx - 1] + in->lon[1] - in->lon[0]);
  const int pole_rows[2][2] = { { 0, 1 }, { ny - 1, ny - 2 } };   // { pole row, its neighbour }
  std::vector<double> cs;       // [pole][c, s][nx]
  if (P.polar) {
    cs.resize((size_t) 4 * nx);
    for (int k = 0; k < 2; k++) {
      const double turn = in->lat[pole_rows[k][0]] < 0 ? -1 : 1;
      for (int ix = 0; ix < nx; ix++) {
        const double a = turn * (in->lon[ix] * (M_PI / 180.0));
        cs[((size_t) 2 * k) * nx + ix] = cos(a);
        cs[((size_t) 2 * k + 1) * nx + ix] = sin(a);
      }
    }
  }

  PrepCall call(ctx);
  if (call.open())
    return 1;
  hipStream_t st = call.st;
  const size_t ncol = (size_t) nx * ny;
  void *d_raw[MPHIP_N3D + MPHIP_N2D] = {};
  double *d_cs = nullptr;
  if (call.mark_begin(1))
    return 1;
  if (P.polar) {
    if (!(d_cs = call.take<double>(cs.size())))
      return 1;
    HIPCHK(hipMemcpyAsync(d_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  for (int i = 0; i < nf; i++) {
    Field &F = fld[i];
    const size_t n = ncol * F.nlev, room = (size_t) nx2 * ny * F.nlev;     // (room: with the periodic column)
    if (F.raw) {
      const size_t bytes = n * (F.raw->type == MPHIP_RAW_SHORT ? sizeof(short) : sizeof(float));
      if (!(F.dev = call.take<float>(room)) || !(d_raw[i] = call.take<char>(bytes)))
        return 1;
      HIPCHK(hipMemcpyAsync(d_raw[i], F.raw->data, bytes, hipMemcpyHostToDevice, st));
    } else if (!(F.dev = F.is3 ? call.upload3(F.src, nx, ny, F.L, room) : call.upload2(F.src, nx, ny, in->sx2, room))) {
      return 1;
    }
  }
  if (call.mark_end() || call.uploads_complete())
    return 1;

  float *dev3[MPHIP_N3D] = {};
  for (int i = 0; i < nf; i++) {
    const Field &F = fld[i];
    if (F.is3)
      dev3[F.f] = F.dev;
    if (!F.raw)
      continue;
    const mphip_raw_t &r = *F.raw;
    const IngestRaw R = { r.scale_factor, r.add_offset, r.fill_f, r.miss_f, r.fill_s, r.miss_s, r.scl, r.lnsp };
    // (a surface field: its y axis in the place of the level)
    const int rows = F.is3 ? ny : 1, lev = F.is3 ? F.nlev : ny;
    const dim3 grid((unsigned) ((nx + kIgTile - 1) / kIgTile), (unsigned) rows, (unsigned) ((lev + kIgTile - 1) / kIgTile));
    if (r.type == MPHIP_RAW_SHORT
          ? call.launch(ingest_decode_kernel<short>, grid, dim3(kIgThreads), 0, (const short *) d_raw[i], F.dev, nx, rows, lev, R)
          : call.launch(ingest_decode_kernel<float>, grid, dim3(kIgThreads), 0, (const float *) d_raw[i], F.dev, nx, rows, lev, R))
      return 1;
  }
  if (what & MPHIP_INGEST_EXTRAPOLATE) {
    IngestColumns C;
    bool any = false;
    for (int i = 0; i < kIgFields; i++)
      any |= (C.f[i] = dev3[kRegridMl[i]]) != nullptr;
    constexpr int per = kIgThreads / 64;
    if (any && call.launch(ingest_extrapolate_kernel, dim3((unsigned) ((ncol + per - 1) / per)), dim3(kIgThreads), 0, C, (int) ncol, np))
      return 1;
  }
  if (P.polar && dev3[MPHIP_U] && dev3[MPHIP_V])
    for (int k = 0; k < 2; k++)
      if (call.launch(ingest_polar_kernel, dim3((unsigned) ((np + 63) / 64)), dim3(64), 0, dev3[MPHIP_U], dev3[MPHIP_V], nx, ny, np,
                      pole_rows[k][0], pole_rows[k][1], (const double *) (d_cs + (size_t) 2 * k * nx),
                      (const double *) (d_cs + ((size_t) 2 * k + 1) * nx)))
        return 1;
  if (P.periodic) {
    IngestCopy C;
    memset(&C, 0, sizeof(C));
    unsigned most = 0;
    for (int i = 0; i < nf; i++) {
      C.p[i] = fld[i].dev;
      C.n[i] = (unsigned) ((size_t) ny * fld[i].nlev);
      most = std::max(most, C.n[i]);
    }
    const unsigned blocks = std::min<unsigned>((most + kIgThreads - 1) / kIgThreads, 1024);
    if (call.launch(ingest_periodic_kernel, dim3(blocks, (unsigned) nf), dim3(kIgThreads), 0, C, nx))
      return 1;
  }
  if (call.mark_begin(2))
    return 1;
  for (int i = 0; i < nf; i++) {
    const Field &F = fld[i];
    if (F.is3 ? call.download3(F.dev, F.dst, nx2, ny, LevelField{ F.nlev, out->sx, out->sy })
              : call.download2(F.dev, F.dst, nx2, ny, out->sx2))
      return 1;
  }
  if (call.close())
    return 1;
  call.write_axes(out, lon2, lat2, p2);
  return 0;
}

size_t mphip_sizeof_met_packed(void) {
  return sizeof(mphip_met_packed_t);
}

// what mphip_unpack_met and mphip_pack_met refuse of the grid of their base description; NULL = accepted
static const char *pack_grid_refusal(const mphip_met_t *m) {
  if (const char *why = grid_dims_refusal(m->nx, m->ny))
    return why;
  if (m->np < 1)
    return "needs one pressure level or more (np < 1)";
  return grid_size_refusal(m->nx, m->ny, std::max(m->np, m->npl));
}

int mphip_unpack_met(mphip_ctx *ctx, const mphip_met_packed_t *in, const mphip_met_t *out) {
  if (!ctx || !in || !out)
    return fail(ctx, "mphip_unpack_met: null argument");
  const mphip_met_t *m = &in->base;
  if (const char *why = pack_grid_refusal(m))
    return fail(ctx, std::string("mphip_unpack_met: ") + why);
  std::string msg;
  if (packed_refusal(in, msg))
    return fail(ctx, "mphip_unpack_met: " + msg);
  int fld[MPHIP_N3D], nf = 0;
  LevelField lev[MPHIP_N3D];      // the levels of the input's grid at the strides of the output's arrays
  for (int f = 0; f < MPHIP_N3D; f++) {
    const LevelField L = level_field(m, f, out);
    if (!in->q3[f] || !out->f3[f] || L.nlev < 1)
      continue;
    if (!regrid_strides_ok(m->ny, L.nlev, L.sx, L.sy))
      return fail(ctx, "mphip_unpack_met: the output strides do not hold the grid");
    fld[nf] = f;
    lev[nf++] = L;
  }
  if (!nf)
    return fail(ctx, "mphip_unpack_met: no field is given as codes in `in` and named in `out`");

  PrepCall call(ctx);
  if (call.open())
    return 1;
  const size_t ncol = (size_t) m->nx * m->ny;
  PackedField B[MPHIP_N3D];
  float *res[MPHIP_N3D];
  if (call.mark_begin(1))
    return 1;
  for (int i = 0; i < nf; i++) {
    B[i] = packed_field(ncol * lev[i].nlev, lev[i].nlev, in->q3[fld[i]]);
    if (!(B[i].blk = call.take<char>(B[i].bytes)) || !(res[i] = call.take<float>(B[i].n))
        || upload_packed(ctx, call.st, B[i], in, fld[i]))
      return 1;
  }
  if (call.mark_end() || call.uploads_complete())
    return 1;
  for (int i = 0; i < nf; i++)
    if (unpack_packed(B[i], in, fld[i], res[i], [&](auto... launch) { return call.launch(launch...); }))
      return 1;
  if (call.mark_begin(2))
    return 1;
  for (int i = 0; i < nf; i++)
    if (call.download3(res[i], (float *) out->f3[fld[i]], m->nx, m->ny, lev[i]))
      return 1;
  return call.close();
}

int mphip_pack_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_met_packed_t *out) {
  if (!ctx || !in || !out)
    return fail(ctx, "mphip_pack_met: null argument");
  if (const char *why = pack_grid_refusal(in))
    return fail(ctx, std::string("mphip_pack_met: ") + why);
  int fld[MPHIP_N3D], nlev[MPHIP_N3D], nf = 0, nlev_sum = 0;
  for (int f = 0; f < MPHIP_N3D; f++) {
    const LevelField L = level_field(in, f);
    if (!in->f3[f] || !out->q3[f] || L.nlev < 1)
      continue;
    if (!out->scl[f] || !out->off[f])
      return fail(ctx, std::string("mphip_pack_met: field ") + kField3Name[f] + " is given as codes without scl or off");
    if (!regrid_strides_ok(in->ny, L.nlev, L.sx, L.sy))
      return fail(ctx, "mphip_pack_met: unsupported meteo strides");
    fld[nf] = f;
    nlev[nf++] = L.nlev;
    nlev_sum += L.nlev;
  }
  if (!nf)
    return fail(ctx, "mphip_pack_met: no field is present in `in` and named as codes in `out`");
  // the extremes: the columns a workgroup stages within 64 KB of LDS at the pitch nlev | 1, up to 64 of them
  const int ncol = in->nx * in->ny;
  int cpb[MPHIP_N3D], nblk[MPHIP_N3D];
  size_t npart = 0;
  for (int i = 0; i < nf; i++) {
    const size_t col_bytes = (size_t) (nlev[i] | 1) * sizeof(float);
    cpb[i] = (int) std::min<size_t>(64, (64 * 1024) / col_bytes);
    if (cpb[i] < 1)
      return fail(ctx, "mphip_pack_met: too many levels for one column in 64 KB of LDS");
    nblk[i] = (ncol + cpb[i] - 1) / cpb[i];
    npart = std::max(npart, (size_t) nblk[i] * (size_t) nlev[i]);
  }

  std::vector<int> bad((size_t) nlev_sum);      // (declared before the call scope: a copy writes it)
  PrepCall call(ctx);
  if (call.open())
    return 1;
  hipStream_t st = call.st;
  float *x[MPHIP_N3D];
  PackedField B[MPHIP_N3D];
  if (call.mark_begin(1))
    return 1;
  for (int i = 0; i < nf; i++) {
    B[i] = packed_field((size_t) ncol * nlev[i], nlev[i], out->q3[fld[i]]);
    if (!(x[i] = call.take<float>(B[i].n)) || !(B[i].blk = call.take<char>(B[i].bytes))
        || call.to_device3(x[i], in->f3[fld[i]], in->nx, in->ny, level_field(in, fld[i])))
      return 1;
  }
  if (call.mark_end())
    return 1;
  // the partials of one field at a time (the stream's order), and the flags of every level of every field
  float *const pmin = call.take<float>(npart), *const pmax = pmin ? call.take<float>(npart) : nullptr;
  int *const pbad = pmax ? call.take<int>(npart) : nullptr, *const d_bad = pbad ? call.take<int>((size_t) nlev_sum) : nullptr;
  if (!d_bad || call.uploads_complete())
    return 1;
  for (int i = 0, at = 0; i < nf; at += nlev[i], i++) {
    const int pitch = nlev[i] | 1;
    if (call.launch_as(4, met_pack_extremes_kernel, dim3((unsigned) nblk[i]), dim3(kPkThreads),
                       (size_t) cpb[i] * pitch * sizeof(float), (const float *) x[i], ncol, nlev[i], cpb[i], pitch, pmin, pmax, pbad)
        || call.launch_as(5, met_pack_reduce_kernel, dim3((unsigned) ((nlev[i] + kPkRedLevels - 1) / kPkRedLevels)),
                          dim3(kPkRedThreads), 0, (const float *) pmin, (const float *) pmax, (const int *) pbad, nblk[i], nlev[i],
                          B[i].scl(), B[i].off(), d_bad + at))
      return 1;
  }
  // a level with a value that is not finite has no code: refused before anything is written
  HIPCHK(hipMemcpyAsync(bad.data(), d_bad, bad.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0, at = 0; i < nf; at += nlev[i], i++)
    for (int k = 0; k < nlev[i]; k++)
      if (bad[(size_t) at + k])
        return fail(ctx, std::string("mphip_pack_met: field ") + kField3Name[fld[i]] + " holds a value that is not finite at level "
                           + std::to_string(k));
  for (int i = 0; i < nf; i++) {
    const PackStream P = pack_stream(B[i].q(), B[i].n, B[i].nlev);
    if (call.launch_as(6, P.table_in_lds ? met_pack_quantise_kernel<true> : met_pack_quantise_kernel<false>, P.grid,
                       dim3(kPkThreads), P.lds, (const float *) x[i], (const double *) B[i].scl(),
                       (const double *) B[i].off(), B[i].q(), P.n, P.nlev, P.head))
      return 1;
  }
  if (call.mark_begin(2))
    return 1;
  for (int i = 0; i < nf; i++) {
    const int f = fld[i];
    HIPCHK(hipMemcpyAsync((void *) out->scl[f], B[i].scl(), (size_t) B[i].nlev * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync((void *) out->off[f], B[i].off(), (size_t) B[i].nlev * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync((void *) out->q3[f], B[i].q(), B[i].n * sizeof(unsigned short), hipMemcpyDeviceToHost, st));
  }
  return call.close();
}

// waits for the uploader thread; 0 = the snapshot is on its way (next_ready recorded)
static int join_uploader(mphip_ctx *ctx) {
  if (ctx->uploader.joinable())
    ctx->uploader.join();
  if (ctx->uploader_rc) {
    ctx->next_pending = false;
    ctx->next.valid = false;
    return fail(ctx, "upload of the prefetched meteo snapshot failed: " + ctx->err);
  }
  return 0;
}

int mphip_commit_met(mphip_ctx *ctx) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  if (!ctx->next_pending)
    return fail(ctx, "no prefetched snapshot to commit");
  HIPCHK(hipSetDevice(ctx->device));
  if (join_uploader(ctx) || flush_meteo(ctx))
    return 1;
  // kernels launched from here on wait for the upload; the host does not
  HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->next_ready, 0));
  ctx->next.valid = true;
  std::swap(ctx->slot[0 ^ ctx->flip], ctx->next);   // the old met0 arrays become the next staging slot
  ctx->flip ^= 1;                                    // old met1 -> met0, prefetched -> met1
  ctx->next.valid = false;
  ctx->next_pending = false;
  if (ctx->pk_next_valid) {
    // the packed grids of (new met0, new met1) are ready on the copy stream (the stepping stream waits for
    // next_ready above): the two sets trade places
    std::swap(ctx->pk, ctx->pk_next);
    ctx->pk_next_valid = false;
    ctx->packed_dirty = false;
    if (axes_follow_met0(ctx))
      return 1;
  } else {
    ctx->packed_dirty = true;
  }
  return 0;
}

int mphip_discard_prefetch(mphip_ctx *ctx) {
  if (!ctx)
    return 1;
  if (!ctx->next_pending)
    return 0;
  HIPCHK(hipSetDevice(ctx->device));
  (void) join_uploader(ctx);
  HIPCHK(hipStreamSynchronize(ctx->copy_stream));
  ctx->next.valid = false;
  ctx->next_pending = false;
  ctx->pk_next_valid = false;
  return 0;
}

int mphip_prefetch_done(mphip_ctx *ctx) {
  if (!ctx || !ctx->next_pending)
    return 1;
  // the uploader thread has handed its last copy to the copy stream and that copy has finished
  return ctx->uploader_done && hipEventQuery(ctx->next_ready) == hipSuccess ? 1 : 0;
}

// intpol_met_time_3d / intpol_met_time_2d (mptrac.c:3112-3170) at the caller's points, from the resident pair
int mphip_intpol_met(mphip_ctx *ctx, long long n, const double *time, long long ntime, const double *p, const double *lon,
                     const double *lat, int nfield, const int *field, double *out) {
  if (!ctx)
    return 1;
  const std::string who = "mphip_intpol_met: ";
  if (n < 0)
    return fail(ctx, who + "n < 0");
  if (!lon || !lat || !out || !time || !field)
    return fail(ctx, who + "a NULL lon, lat, out, time or field");
  if (ntime != 1 && ntime != n)
    return fail(ctx, who + "ntime must be 1 or n");
  if (nfield < 1 || nfield > kIntpolMaxFields)
    return fail(ctx, who + "nfield must be in 1 ... 32");
  const MetSlot &s0 = ctx->slot[0 ^ ctx->flip], &s1 = ctx->slot[1 ^ ctx->flip];
  if (!s0.valid || !s1.valid)
    return fail(ctx, who + "a meteo slot without a snapshot");
  if (s0.time == s1.time)
    return fail(ctx, who + "time0 == time1");
  IntpolArgs I = {};
  for (int k = 0; k < nfield; k++) {
    const bool is2 = (field[k] & MPHIP_INTPOL_2D) != 0;
    const int f = field[k] & ~MPHIP_INTPOL_2D;
    if (f < 0 || f >= (is2 ? (int) MPHIP_N2D : (int) MPHIP_N3D))
      return fail(ctx, who + "field index " + std::to_string(field[k]) + " out of range");
    const char *name = is2 ? kField2Name[f] : kField3Name[f];
    if (!is2 && field_on_model_levels(f))
      return fail(ctx, who + "model-level field " + name + " is out of scope");
    if (!(is2 ? s0.has2[f] && s1.has2[f] : s0.has3[f] && s1.has3[f]))
      return fail(ctx, who + "field " + name + " was not uploaded with both resident snapshots");
    I.field[k] = is2 ? (f | kIntpol2D) : f;
    I.f0[k] = is2 ? s0.f2[f].p : s0.f3[f].p;
    I.f1[k] = is2 ? s1.f2[f].p : s1.f3[f].p;
    I.need_p |= !is2;
  }
  if (I.need_p && !p)
    return fail(ctx, who + "a NULL p with a pressure-level field");
  // the kernel keeps the three axes and their reciprocal widths in LDS: 16 bytes per node, 64 KB per workgroup
  if (2 * (size_t) (ctx->nx + ctx->ny + ctx->npl) * sizeof(double) > 64 * 1024)
    return fail(ctx, who + "the axes of the meteo grid (" + std::to_string(ctx->nx + ctx->ny + ctx->npl)
                + " nodes) do not fit 64 KB of LDS (at most 4096 nodes)");
  if (n == 0)
    return 0;
  HIPCHK(hipSetDevice(ctx->device));
  if (axes_follow_met0(ctx))
    return 1;
  DevMet M = {};
  M.axes = ctx->d_axes.p;
  M.nx = ctx->nx;
  M.ny = ctx->ny;
  M.np = ctx->npl;
  M.coord_type = ctx->coord_type;
  M.time0 = s0.time;
  M.time1 = s1.time;
  M.lat_ascending = ctx->h_lat[(ctx->ny - 1) >> 1] < ctx->h_lat[((ctx->ny - 1) >> 1) + 1];
  M.p_ascending = ctx->h_p[(ctx->npl - 1) >> 1] < ctx->h_p[((ctx->npl - 1) >> 1) + 1];
  const size_t lds = 2 * (size_t) (M.nx + M.ny + M.np) * sizeof(double);   // (no pressure table: lut_size = 0)
  const size_t chunk = (size_t) std::min<long long>(n, ctx->intpol_chunk);
  HIPCHK(ctx->d_ip_in.reserve(4 * chunk));
  HIPCHK(ctx->d_ip_out.reserve((size_t) nfield * chunk));
  double *const d_time = ctx->d_ip_in.p, *const d_p = d_time + chunk, *const d_lon = d_p + chunk, *const d_lat = d_lon + chunk;
  I.nfield = nfield;
  I.time_all = time[0];
  I.out = ctx->d_ip_out.p;
  I.out_stride = (long long) chunk;
  for (size_t first = 0; first < (size_t) n; first += chunk) {
    const size_t m = std::min(chunk, (size_t) n - first), bytes = m * sizeof(double);
    if (ntime == n)
      HIPCHK(hipMemcpyAsync(d_time, time + first, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (I.need_p)
      HIPCHK(hipMemcpyAsync(d_p, p + first, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_lon, lon + first, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_lat, lat + first, bytes, hipMemcpyHostToDevice, ctx->stream));
    I.time = ntime == n ? d_time : nullptr;
    I.p = d_p;
    I.lon = d_lon;
    I.lat = d_lat;
    I.n = (long long) m;
    hipEvent_t e1 = nullptr;   // (mphip_profile_begin / _end around calls of this function alone: the time of its kernel)
    if (prof_pair(ctx, ctx->stream, &e1))
      return 1;
    hipLaunchKernelGGL(intpol_points_kernel, dim3(grid_for((long long) m)), dim3(256), lds, ctx->stream, M, I);
    HIPCHK(hipGetLastError());
    if (e1)
      HIPCHK(hipEventRecord(e1, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(out + first, (size_t) n * sizeof(double), ctx->d_ip_out.p, chunk * sizeof(double), bytes,
                            (size_t) nfield, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_update_atm(mphip_ctx *ctx, long long np, long long ip0, long long np_total, int nq, const double *time,
                     const double *p, const double *lon, const double *lat, const double *const *q) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx || np < 0 || nq < 0 || nq > MPHIP_NQ_MAX || ip0 < 0 || np_total < ip0 + np)
    return fail(ctx, "bad particle counts");
  if (np > 2147483647LL)
    return fail(ctx, "too many particles for one device context");
  if (np && (!time || !p || !lon || !lat || (nq && !q)))
    return fail(ctx, "null particle array");
  HIPCHK(hipSetDevice(ctx->device));
  const bool fresh = (np != ctx->np || nq != ctx->nq || !ctx->d_arr[0].p);
  if (fresh) {
    const size_t n = (size_t) std::max<long long>(np, 1);
    for (int k = 0; k < 4 + MPHIP_NQ_MAX; k++) {
      const size_t want = k < 4 + nq ? n : 0;
      HIPCHK(ctx->d_arr[k].resize(want));
      HIPCHK(ctx->d_alt[k].resize(want));
    }
    for (int k = 0; k < 3; k++) {
      HIPCHK(ctx->d_uvwp[k].resize(n));
      HIPCHK(ctx->d_uvwp_alt[k].resize(n));
      HIPCHK(hipMemsetAsync(ctx->d_uvwp[k].p, 0, n * sizeof(float), ctx->stream));   // calloc'ed cache_t
    }
    HIPCHK(ctx->d_dt.resize(n));
    HIPCHK(ctx->d_dt_alt.resize(n));
    HIPCHK(hipMemsetAsync(ctx->d_dt.p, 0, n * sizeof(double), ctx->stream));
    HIPCHK(ctx->d_ext.resize(n));
    HIPCHK(ctx->d_ext_alt.resize(n));
    for (int k = 0; k < 2; k++) {
      HIPCHK(ctx->d_keys[k].resize(n));
      HIPCHK(ctx->d_vals[k].resize(n));
    }
    HIPCHK(ctx->d_cell.resize(n));
    // the per-particle buffers of the sort ahead and of the order repair come back at the new count on first use
    for (int k = 0; k < 2; k++) {
      ctx->ahead_keys[k].release();
      ctx->ahead_vals[k].release();
      ctx->rep_mk[k].release();
      ctx->rep_mi[k].release();
    }
    ctx->ahead_dt.release();
    ctx->rep_sk.release();
    ctx->rep_si.release();
    ctx->rep_fk.release();
    ctx->rep_fv.release();
    ctx->d_iso.release();
    ctx->d_iso_alt.release();
    ctx->d_kz.release();
    ctx->d_kz_alt.release();
    ctx->sorted_buf = -1;
    ctx->stored_is_sorted = false;
  }
  ctx->depo_busy_valid = false;
  ctx->meteo_pending = false;   // the uploaded quantity arrays replace whatever module_meteo would have written
  if (!fresh && restore_external_order(ctx))   // keep cache->uvwp with its slot across a re-upload
    return 1;
  ctx->ext_identity = true;
  ctx->stored_is_sorted = false;     // (the caller's particles: in no order this library knows of)
  ctx->steps_since_resort = 1 << 30;
  ctx->np = np;
  ctx->nq = nq;
  ctx->ip0 = ip0;
  ctx->np_total = np_total;
  const double *src[4] = { time, p, lon, lat };
  if (np) {
    const void *all[4 + MPHIP_NQ_MAX] = { time, p, lon, lat };
    for (int iq = 0; iq < nq; iq++)
      all[4 + iq] = q[iq];
    pin_host_span(ctx, all, 4 + nq, (size_t) np * sizeof(double));
  }
  for (int k = 0; k < 4 && np; k++)
    HIPCHK(hipMemcpyAsync(ctx->d_arr[k].p, src[k], (size_t) np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  for (int iq = 0; iq < nq && np; iq++) {
    if (!q[iq])
      return fail(ctx, "null quantity array");
    HIPCHK(hipMemcpyAsync(ctx->d_arr[4 + iq].p, q[iq], (size_t) np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_update_quantity(mphip_ctx *ctx, int iq, const double *q) {
  if (!ctx || !q)
    return fail(ctx, "null argument");
  if (iq < 0 || iq >= ctx->nq)
    return fail(ctx, "no such quantity");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))   // (a pending module_meteo may be about to write this array)
    return 1;
  if (ctx->np == 0)
    return 0;
  const size_t bytes = (size_t) ctx->np * sizeof(double);
  if (ctx->ext_identity) {
    HIPCHK(hipMemcpyAsync(ctx->d_arr[4 + iq].p, q, bytes, hipMemcpyHostToDevice, ctx->stream));
  } else {   // through the alternate buffer (free between two sorts), then into the stored order
    HIPCHK(hipMemcpyAsync(ctx->d_alt[4 + iq].p, q, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(gather_by_ext_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, ctx->d_alt[4 + iq].p,
                       ctx->d_ext.p, ctx->d_arr[4 + iq].p, ctx->np);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_get_atm(mphip_ctx *ctx, double *time, double *p, double *lon, double *lat, double *const *q) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))
    return 1;
  // The caller's order is produced in the alternate buffers (free between two sorts); the resident
  // arrays keep their internal order, so an output costs one scatter pass and no re-sort.
  const DevBuf<double> *srcs = ctx->d_arr;
  if (!ctx->ext_identity && ctx->np) {
    PermArgs g = perm_args(ctx, false);
    if (permute_random(ctx, g, ctx->d_ext.p, ctx->np, true))
      return 1;
    srcs = ctx->d_alt;
  }
  double *dst[4] = { time, p, lon, lat };
  if (ctx->np) {
    const void *all[4 + MPHIP_NQ_MAX] = { time, p, lon, lat };
    for (int iq = 0; iq < ctx->nq; iq++)
      all[4 + iq] = q ? q[iq] : nullptr;
    pin_host_span(ctx, all, 4 + ctx->nq, (size_t) ctx->np * sizeof(double));
  }
  for (int k = 0; k < 4; k++)
    if (dst[k] && ctx->np)
      HIPCHK(hipMemcpyAsync(dst[k], srcs[k].p, (size_t) ctx->np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  for (int iq = 0; iq < ctx->nq; iq++)
    if (q && q[iq] && ctx->np)
      HIPCHK(hipMemcpyAsync(q[iq], srcs[4 + iq].p, (size_t) ctx->np * sizeof(double), hipMemcpyDeviceToHost,
                            ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_update_cache(mphip_ctx *ctx, const float *uvwp, const uint64_t *rng_ctr) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if (rng_ctr)
    ctx->rng_ctr = *rng_ctr;
  if (uvwp && restore_external_order(ctx))
    return 1;
  if (uvwp && ctx->np) {
    std::vector<float> tmp((size_t) ctx->np);
    for (int k = 0; k < 3; k++) {
      for (long long i = 0; i < ctx->np; i++)
        tmp[(size_t) i] = uvwp[3 * (size_t) i + k];
      HIPCHK(hipMemcpy(ctx->d_uvwp[k].p, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  return 0;
}

int mphip_get_cache(mphip_ctx *ctx, float *uvwp, double *dt, uint64_t *rng_ctr) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if ((uvwp || dt) && restore_external_order(ctx))
    return 1;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (rng_ctr)
    *rng_ctr = ctx->rng_ctr;
  if (uvwp && ctx->np) {
    std::vector<float> tmp((size_t) ctx->np);
    for (int k = 0; k < 3; k++) {
      HIPCHK(hipMemcpy(tmp.data(), ctx->d_uvwp[k].p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (long long i = 0; i < ctx->np; i++)
        uvwp[3 * (size_t) i + k] = tmp[(size_t) i];
    }
  }
  if (dt && ctx->np)
    HIPCHK(hipMemcpy(dt, ctx->d_dt.p, (size_t) ctx->np * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int mphip_update_iso(mphip_ctx *ctx, const double *iso_var, const double *iso_ts, const double *iso_ps, int iso_n) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if (iso_var && ctx->np) {
    if (restore_external_order(ctx) || ensure_iso(ctx))
      return 1;
    HIPCHK(hipMemcpyAsync(ctx->d_iso.p, iso_var, (size_t) ctx->np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  if (iso_ts && iso_ps) {
    if (iso_n < 1)
      return fail(ctx, "Could not read any data!");   // module_isosurf_init, mptrac.c:4943-4944
    HIPCHK(ctx->d_iso_ts.resize((size_t) iso_n));
    HIPCHK(ctx->d_iso_ps.resize((size_t) iso_n));
    HIPCHK(hipMemcpyAsync(ctx->d_iso_ts.p, iso_ts, (size_t) iso_n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_iso_ps.p, iso_ps, (size_t) iso_n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ctx->iso_n = iso_n;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_get_iso(mphip_ctx *ctx, double *iso_var) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  if (iso_var && ctx->np) {
    if (!ctx->d_iso.p)
      return fail(ctx, "cache->iso_var is not on the device (no isosurface mode has run)");
    if (restore_external_order(ctx))
      return 1;
    HIPCHK(hipMemcpyAsync(iso_var, ctx->d_iso.p, (size_t) ctx->np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

int mphip_run_timestep(mphip_ctx *ctx, double t) {
  if (!ctx)
    return 1;
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  HIPCHK(hipSetDevice(ctx->device));
  const mphip_ctl_t &c = ctx->ctl;
  const StepPlan P = plan_step(ctx, t);
  if (settle_meteo(ctx, P.due.meteo))
    return 1;

  // module_isosurf_init and module_advect_init at the first call (mptrac.c:7863-7870)
  if (t == c.t_start) {
    unsigned init = 0;
    if (c.isosurf >= 1 && c.isosurf <= 3)
      init |= MPHIP_MOD_ISOSURF_INIT;
    if (c.advect_vert_coord == 1)
      init |= MPHIP_MOD_ADVECT_INIT;
    if (init && launch_step(ctx, init, t))
      return 1;
  }

  // module_timesteps + module_sort (mptrac.c:7877-7881).  The reference
  // permutes atm but not cache->dt, so on sort steps dt is computed per slot
  // before the sort and read back per slot afterwards.
  if (P.due.sort) {
    if (restore_external_order(ctx) || do_sort(ctx, &t))
      return 1;
  } else if (ctx->locality_interval > 0 && ctx->steps_since_resort >= ctx->locality_interval) {
    if (locality_sort(ctx))
      return 1;
  }
  if (ctx->steps_since_resort < (1 << 29))
    ctx->steps_since_resort++;
  ctx->rng_ctr += P.per_step;
  unsigned mask = P.mask;
  const unsigned tail = P.tail;
  // module_meteo (mptrac.c:7921-7924) sits between the final module_position and the loss / decay /
  // mixing / deposition modules; those neither move particles nor touch a quantity it sets, so it
  // runs after them here (own kernel, every particle)
  // module_sort of the next step can start as soon as this step's particles have moved (sort_ahead)
  const double t_next = t + c.direction * c.dt_mod;
  const bool sort_next = ctx->sort_ahead && ctx->np > 0 && ctx->ext_identity && c.sort_dt > 0
    && fmod(t_next, c.sort_dt) == 0 && c.direction * (t_next - c.t_stop) <= 0;
  // the chemistry (module_chem_grid, module_oh_chem, module_h2o2_chem, module_tracer_chem: launch_chem, own kernels)
  // sits between module_mixing and module_wet_depo: with it the step's launch stops before the deposition modules,
  // which follow in a launch of their own
  const bool chem = step_chem_on(c);
  // module_radio_depo (mphip_set_radio_depo) is a launch of its own behind the tail, on the stored dt: the split path too
  const bool rdepo = step_radio_depo_on(ctx);
  // (the busy list of the launch that moved the particles, where the step's deposition launch has just used it)
  auto radio_depo_step = [&]() {
    const bool listed = ctx->depo_busy_last && ctx->depo_busy_last_mask == depo_bits(c);
    const unsigned char *busy = listed ? ctx->depo_busy_last : nullptr;
    ctx->depo_busy_last = nullptr;
    return launch_radio_depo(ctx, t, busy);
  };
  if (!P.due.mixing && !chem && !rdepo) {
    if (launch_step(ctx, mask | tail, t, P.rng))
      return 1;
    if (sort_next && ahead_launch(ctx, t_next))
      return 1;
    return P.due.meteo ? schedule_meteo(ctx) : 0;
  }
  if ((tail || chem) && (mask & MPHIP_MOD_TIMESTEPS))
    mask |= kStoreDt;
  if (!P.due.mixing) {
    if (launch_step(ctx, mask, t, P.rng))
      return 1;
    if (sort_next && ahead_launch(ctx, t_next))
      return 1;
    if ((chem && launch_chem(ctx, t)) || (tail && launch_step(ctx, tail, t)) || (rdepo && radio_depo_step()))
      return 1;
    return P.due.meteo ? schedule_meteo(ctx) : 0;
  }
  // the keys of the sort ahead, its module_timesteps and module_mixing's box index from the launch that moves the
  // particles (EmitKeys) instead of a kernel of their own behind it, where an instantiation for it exists
  EmitKeys ek;
  memset(&ek, 0, sizeof(ek));
  bool emitted = false;
  if (sort_next && ctx->ahead_box && ctx->emit_keys) {
    MixPlan plan;
    bool act = false;
    if (mixing_plan(ctx, t, &plan, &act) || ahead_ensure(ctx))
      return 1;
    if (act) {
      ek.keys = ctx->ahead_keys[0].p;
      ek.dt_next = ctx->ahead_dt.p;
      ek.cell = ctx->d_cell.p;
      ek.grid = plan.box.grid;
      ek.box_t0 = plan.box.t0;
      ek.box_t1 = plan.box.t1;
      ek.ens = plan.box.ens;
      ek.ngrid = plan.box.ngrid;
      ek.direction = (double) c.direction;
      ek.t_start = c.t_start;
      ek.t_stop = c.t_stop;
      ek.t_next = t_next;
      constexpr unsigned kDepo = MPHIP_MOD_WET_DEPO | MPHIP_MOD_DRY_DEPO;
      // (the flags measured against a deposition launch that decides from dt, time, p itself: profiles/r06_ab_depo_flags.txt)
      if ((tail & kDepo) && !(tail & ~kDepo) && ctx->compact_depo) {   // the deposition launch behind module_mixing will be depo_kernel
        HIPCHK(ctx->d_depo_busy.reserve((size_t) ctx->np));
        ek.depo_busy = ctx->d_depo_busy.p;
        ek.depo_mask = tail;
      }
    }
  }
  if (launch_step(ctx, mask, t, P.rng, 1, 0, 0, &ek, &emitted))
    return 1;
  bool cells_ready = false;
  if (sort_next) {   // ... beside module_mixing and the deposition launch
    MixPlan plan;
    if (mixing_plan(ctx, t, &plan, &cells_ready))
      return 1;
    const BoxArgs box = { ctx->d_cell.p, plan.box.grid, plan.box.t0, plan.box.t1, plan.box.ens, plan.box.ngrid };
    if (!ctx->ahead_box)
      cells_ready = false;
    if (ahead_launch(ctx, t_next, cells_ready ? &box : nullptr, emitted && cells_ready))
      return 1;
  }
  if (do_mixing(ctx, t, cells_ready))
    return 1;
  if (chem && launch_chem(ctx, t))
    return 1;
  if (tail && launch_step(ctx, tail, t))
    return 1;
  if (rdepo && radio_depo_step())
    return 1;
  return P.due.meteo ? schedule_meteo(ctx) : 0;
}

// mphip_run_timesteps: n calls of mphip_run_timestep at t_first, t_first + stride, ... (stride = direction * DT_MOD,
// accumulated as the loop of trac.c:208 accumulates it).  Runs of steps with nothing between them -- no module_sort,
// no mixing, no module_meteo, no rarely used module, convection (if any) in every step, the internal re-sort not
// due -- and a lean instantiation of their module set go to the device as ONE launch in which every particle takes
// its steps one after the other: at small particle counts a step is shorter than a kernel launch.  Everything else
// takes the steps one by one; the results are the same either way (tests/test_gpu_parity.py).
int mphip_run_timesteps(mphip_ctx *ctx, double t_first, int nsteps) {
  if (!ctx)
    return 1;
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  if (nsteps < 0)
    return fail(ctx, "mphip_run_timesteps: negative step count");
  const mphip_ctl_t &c = ctx->ctl;
  const double stride = c.direction * c.dt_mod;
  double t = t_first;
  int done = 0;
  while (done < nsteps) {
    // how many steps from here on can share a launch?
    int batch = 0;
    // module_meteo (lazy: evaluated when its values can be seen, dropped when the next step schedules it again --
    // mphip_run_timestep) lets a batch run on, except that it must be evaluated between a step that schedules it and a
    // step that does not: a batch ends behind such a step.  (module_meteo without a quantity to fill does nothing.)
    const bool meteo = meteo_requested(c);
    auto meteo_at = [&](double tt) { return meteo && due_at(c, tt).meteo; };
    // module_sort and module_mixing run at multiples of SORT_DT / MIXING_DT: such a step takes the single-step path
    // (which sorts, or splits its launch around the mixing), the steps between two of them can share launches
    // (module_convection with CONV_DT > 0 likewise: due steps on their own, the steps between without it)
    auto scheduled = [&](double tt) {
      const StepDue d = due_at(c, tt);
      return d.sort || d.mixing || (d.conv && c.conv_dt > 0);
    };
    const bool quiet = ctx->multi_step && ctx->np > 0 && t != c.t_start && !scheduled(t)
      && c.advect > 0   // (every integrator has its multi-step instantiations; without module_advect: single steps)
      && !ctx->fused_perm
      && !ctx->force_generic
      && !step_chem_on(c)    // (module_chem_grid, module_oh_chem, module_h2o2_chem, module_tracer_chem are launches of
                             // their own: single steps)
      && !step_radio_depo_on(ctx);   // (module_radio_depo likewise, behind the tail)
    // the internal re-sort falls due at this step: the launch that takes the steps behind it can do its gather on the
    // way (the pass over every array and the single-step launch saved), if it is a lean pressure-level multi-step one.
    // The batch is then sized as behind the sort; whatever cannot take the fold goes the way of a batch of 0 --
    // mphip_run_timestep, which sorts with a pass of its own.
    // (model-level winds and the general kernels -- `quiet` excludes the option generic_kernel -- have no such
    // instantiation: ruled out here, so that their due step goes to mphip_run_timestep without being planned twice)
    const bool fold = quiet && ctx->fold_resort && ctx->locality_interval > 0
      && ctx->steps_since_resort >= ctx->locality_interval && !ctx->ext_identity
      && !ml_winds(c) && !ctx->d_iso.p && !ctx->d_kz.p && ctx->lds_tile <= 0;
    if (quiet) {
      batch = nsteps - done;
      if (ctx->locality_interval > 0)
        batch = std::min(batch, fold ? ctx->locality_interval : ctx->locality_interval - ctx->steps_since_resort);
      batch = std::min(batch, ctx->multi_step);
      double tt = t;
      for (int j = 0; j < batch; j++) {
        if (j > 0 && scheduled(tt)) {   // the batch ends before this step
          batch = j;
          break;
        }
        const double tn = tt + stride;
        if (meteo_at(tt) && (!ctx->lazy_meteo || !meteo_at(tn))) {   // ... behind this one
          batch = j + 1;
          break;
        }
        tt = tn;
      }
    }
    // the plan of mphip_run_timestep for the first step serves all `batch` steps, if an instantiation takes them
    // (model-level winds: only once a single-step launch has allocated and seeded the search hints, d_kz)
    StepPlan P{};
    if (batch > 1) {
      HIPCHK(hipSetDevice(ctx->device));
      if (ensure_packed(ctx))
        return 1;
      P = plan_step(ctx, t);
      const unsigned sel = step_kernel_mask(ctx, P.mask | P.tail, batch);
      if (sel == kNoStepKernel || (ml_winds(c) && !ctx->d_kz.p) || (fold && !step_kernel_stores_once(sel)))
        batch = 1;
    }
    if (batch < 2) {
      if (mphip_run_timestep(ctx, t))
        return 1;
      t += stride;
      done++;
      continue;
    }
    if (settle_meteo(ctx, meteo_at(t)))
      return 1;
    if (fold) {   // (sort and launch in this iteration: nothing else sees the hand-over)
      int cur = 0;
      if (check_fields(ctx, P.mask | P.tail)   // (what launch_step could refuse, before the arrays change places)
          || locality_sort_keys(ctx, &cur) || locality_sort_apply(ctx, cur, true))
        return 1;
    }
    const int rc = launch_step(ctx, P.mask | P.tail, t, P.rng, batch, stride, P.per_step);
    ctx->fold_perm = nullptr;
    if (rc)
      return 1;
    ctx->rng_ctr += P.per_step * (uint64_t) batch;
    if (ctx->steps_since_resort < (1 << 29))
      ctx->steps_since_resort += batch;
    double t_last = t;
    for (int k = 0; k < batch; k++) {
      t_last = t;
      t += stride;
    }
    done += batch;
    if (meteo_at(t_last) && schedule_meteo(ctx))   // (only the last step of a batch can leave one to be seen)
      return 1;
  }
  return 0;
}

int mphip_module(mphip_ctx *ctx, unsigned modules, double t) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))
    return 1;
  switch (modules) {
  case MPHIP_MOD_SORT:
    return do_sort(ctx);
  case MPHIP_MOD_MIXING:
    return do_mixing(ctx, t);
  case MPHIP_MOD_METEO:
    return launch_meteo(ctx);
  case MPHIP_MOD_OH_CHEM:
    return launch_oh(ctx);
  case MPHIP_MOD_CHEM_GRID:
    return do_chem_grid(ctx, t);
  case MPHIP_MOD_H2O2_CHEM:
    return launch_h2o2(ctx);
  case MPHIP_MOD_TRACER_CHEM:
    return launch_tracer_chem(ctx);
  case MPHIP_MOD_RADIO_DEPO:   // alone, on the stored dt (whether or not the step's switch is on)
    return launch_radio_depo(ctx, t, nullptr);
  }
  // module_radio_decay: the tail of a step-kernel launch (alone: on the stored dt), with whatever activities are registered
  if (modules & MPHIP_MOD_RADIO_DECAY) {
    modules &= ~(unsigned) MPHIP_MOD_RADIO_DECAY;
    if (radio_any(ctx))
      modules |= kRadioDecay;
    else if (!modules)
      return 0;
  }
  if (modules & ~(kParticleBits | kRadioDecay))
    return fail(ctx, "module_sort / module_mixing / module_meteo / module_chem_grid / module_oh_chem / module_h2o2_chem "
                     "/ module_tracer_chem / module_radio_depo must be called on their own");
  uint64_t per_step = 0;
  const RngCtr rng = rng_counters(modules, (uint64_t) ctx->np_total, ctx->rng_ctr, &per_step);
  ctx->rng_ctr += per_step;
  if (modules & MPHIP_MOD_TIMESTEPS)
    modules |= kStoreDt;
  return launch_step(ctx, modules, t, rng);
}

int mphip_get_sort(mphip_ctx *ctx, double *keys, int *perm) {
  if (!ctx || ctx->sorted_buf < 0)
    return fail(ctx, "module_sort has not been run");
  HIPCHK(hipSetDevice(ctx->device));
  const long long n = ctx->np;
  if (perm)
    HIPCHK(hipMemcpyAsync(perm, ctx->d_vals[ctx->sorted_buf].p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
  if (keys) {
    DevBuf<double> d_tmp;
    HIPCHK(d_tmp.resize((size_t) n));
    hipLaunchKernelGGL(keys_to_double_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->stream,
                       ctx->d_keys[ctx->sorted_buf].p, d_tmp.p, n);
    HIPCHK(hipMemcpyAsync(keys, d_tmp.p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_get_sort_counts(mphip_ctx *ctx, long long *repaired, long long *scratch, long long *undone) {
  if (!ctx || !repaired || !scratch)
    return fail(ctx, "null argument");
  *repaired = ctx->sorts_repaired;
  *scratch = ctx->sorts_scratch;
  if (undone)
    *undone = ctx->sorts_undone;
  return 0;
}

int mphip_grid_sums(mphip_ctx *ctx, double t, int *cnt, double *mean, double *sigma) {
  if (!ctx || !cnt || !mean || !sigma)
    return fail(ctx, "null argument");
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))
    return 1;
  const mphip_ctl_t &c = ctx->ctl;
  const size_t ncell = (size_t) c.grid_nx * c.grid_ny * c.grid_nz;
  const size_t total = ncell * (size_t) (1 + 2 * ctx->nq);
  if (reserve(ctx, ctx->d_sums, total))
    return 1;
  const bool ordered = ctx->deterministic_sums != 0;
  const DevAtm a = dev_atm(ctx);
  const GridKernel kern = { ctx->d_grid_kernel.p, ctx->d_grid_kernel.p ? ctx->d_grid_kernel.p + ctx->grid_nk : nullptr, a.p,
                            ctx->grid_nk };
  const BoxGrid G = { c.grid_lon0, c.grid_lon1, c.grid_lat0, c.grid_lat1, c.grid_z0, c.grid_z1, c.grid_nx, c.grid_ny,
                      c.grid_nz };
  const GridBoxArgs gbox = { G, t - 0.5 * c.dt_mod, t + 0.5 * c.dt_mod, a.time, a.lon, a.lat, a.p };
  if (ctx->np && !ordered)   // (the ordered sums compute the box index on their way)
    hipLaunchKernelGGL(box_index_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, a, G, gbox.t0, gbox.t1,
                       ctx->d_cell.p, (const double *) nullptr, 0);
  if (ordered) {
    GridVals vals;
    for (int iq = 0; iq < ctx->nq; iq++)
      vals.q[iq] = a.q[iq];
    vals.nq = ctx->nq;
    vals.kern = kern;
    vals.rec = nullptr;
    // the particles' values as records (see GridVals): worth the extra pass from two quantities on; without the
    // memory for it the sums gather from the arrays
    if (ctx->nq >= 2 && ctx->np > 0 && ctx->grid_records) {
      const size_t need = (size_t) ctx->np * (size_t) ctx->nq;
      if (ctx->d_rec.try_reserve(need)) {
        hipLaunchKernelGGL(grid_records_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, vals, ctx->np, ctx->d_rec.p);
        vals.rec = ctx->d_rec.p;
      }
    }
    // [counts | sums of q | sums of q^2], as grid_accumulate_kernel
    if (ordered_cell_sums(ctx, vals, 2 * ctx->nq, c.grid_nz, ncell, ctx->d_sums.p + ncell, (int *) nullptr, ctx->d_sums.p, true,
                          &gbox))
      return 1;
  } else {
    HIPCHK(hipMemsetAsync(ctx->d_sums.p, 0, total * sizeof(double), ctx->stream));
    if (ctx->np) {
      const AccumGeom g = accum_geom(ctx, 1 + 2 * ctx->nq);
      hipLaunchKernelGGL(grid_accumulate_kernel, dim3(g.nblocks), dim3(256), g.lds, ctx->stream, a, ctx->d_cell.p, ctx->nq,
                         ncell, ctx->d_sums.p, g.T, g.per_block, kern);
    }
  }
  HIPCHK(hipGetLastError());
  if (run_allreduce(ctx, ctx->d_sums.p, total))
    return 1;
  // through a page-locked staging buffer of the context: from pageable memory the 3.6 MB of a 360 x 180 grid
  // with three quantities took 0.3 ms of the output's 0.9
  HIPCHK(ctx->h_sums.reserve(total));
  double *h = ctx->h_sums.p;
  HIPCHK(hipMemcpyAsync(h, ctx->d_sums.p, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ncell; i++)
    cnt[i] = (int) h[i];
  memcpy(mean, h + ncell, ncell * (size_t) ctx->nq * sizeof(double));
  memcpy(sigma, h + ncell * (size_t) (1 + ctx->nq), ncell * (size_t) ctx->nq * sizeof(double));
  return 0;
}

// ---- analysis outputs: write_csi / write_prof / write_sample / write_station particle loops ---------------------------

namespace {

int ana_common(mphip_ctx *ctx, const char *what) {
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  if (ctx->ctl.met_coord_type != 0)
    return fail(ctx, std::string(what) + ": Only lat/lon grid supported");
  HIPCHK(ctx->d_ana_flags.reserve(8));
  return 0;
}

bool is_meteo_quantity(const mphip_ctx *ctx, int iq) {
  for (int k = 0; k < MPHIP_NMQ; k++)
    if (iq >= 0 && ctx->ctl.qnt_met[k] == iq)
      return true;
  return false;
}

// the call's weighting function on the device (nk < 2: none)
int ana_kernel_fn(mphip_ctx *ctx, int nk, const double *kz, const double *kw, KernelFn *K) {
  K->kz = K->kw = nullptr;
  K->nk = 0;
  if (nk < 2)
    return 0;
  if (!kz || !kw)
    return fail(ctx, "bad kernel function");
  for (int k = 1; k < nk; k++)
    if (kz[k] < kz[k - 1])
      return fail(ctx, "height levels of the kernel function must be ascending");
  HIPCHK(ctx->d_ana_kernel.reserve(2 * (size_t) nk));
  HIPCHK(hipMemcpyAsync(ctx->d_ana_kernel.p, kz, (size_t) nk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->d_ana_kernel.p + nk, kw, (size_t) nk * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  K->kz = ctx->d_ana_kernel.p;
  K->kw = ctx->d_ana_kernel.p + nk;
  K->nk = nk;
  return 0;
}

// (d_rec, a value per stored particle / per record, is the record buffer of mphip_grid_sums: there the gridded sums
// do without it when it cannot be had; the analysis outputs need it, reserve(ctx, ctx->d_rec, ...))

// Exclusive scan of the np + 1 counts in ctx->d_marks (the last one is zero): offset of element e afterwards =
// d_marks[e] + chunk_off[e >> shift]; the total (offset of element np) goes to d_ana_flags[1].
struct MarkScan {
  uint32_t *chunk_off;
  int shift;
};

int ensure_marks(mphip_ctx *ctx, MarkScan *M) {
  const size_t m = (size_t) ctx->np + 1;
  HIPCHK(ctx->d_marks.reserve(m + kScanThreads));
  M->chunk_off = ctx->d_marks.p + m;
  M->shift = m <= (size_t) kScanThreads * kScanPerLarge * kScanThreads ? 14 : 16;
  if (((m + ((size_t) 1 << M->shift) - 1) >> M->shift) > (size_t) kScanThreads)
    return fail(ctx, "too many particles for the scan of the analysis outputs");
  return 0;
}

int scan_marks(mphip_ctx *ctx, const MarkScan &M) {
  const size_t m = (size_t) ctx->np + 1;
  const int nchunks = (int) ((m + ((size_t) 1 << M.shift) - 1) >> M.shift);
  if (M.shift == 14)
    hipLaunchKernelGGL(sort_scan_local_kernel<kScanPerLarge>, dim3(nchunks), dim3(kScanThreads), 0, ctx->stream, ctx->d_marks.p,
                       m, M.chunk_off, (const uint32_t *) nullptr, 0);
  else
    hipLaunchKernelGGL(sort_scan_local_kernel<64>, dim3(nchunks), dim3(kScanThreads), 0, ctx->stream, ctx->d_marks.p, m,
                       M.chunk_off, (const uint32_t *) nullptr, 0);
  hipLaunchKernelGGL(sort_scan_chunks_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, M.chunk_off, nchunks);
  hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->d_marks.p, M.chunk_off, M.shift, ctx->np,
                     ctx->d_ana_flags.p + 1);
  HIPCHK(hipGetLastError());
  return 0;
}

// geo2cart(0, lon, lat, x) of output.c with the host's C library
void geo2cart_host(double lon, double lat, double *x) {
  const double r = 6367.421 + 0.0, phi = lat * (M_PI / 180.0), lam = lon * (M_PI / 180.0);
  x[0] = r * cos(phi) * cos(lam);
  x[1] = r * cos(phi) * sin(lam);
  x[2] = r * sin(phi);
}

}   // namespace

int mphip_box_sums(mphip_ctx *ctx, const mphip_box_t *box, double t, int qnt, int nmember, int qnt_member, int nk,
                   const double *kz, const double *kw, double *sum) {
  if (!ctx || !box || !sum)
    return fail(ctx, "null argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (ana_common(ctx, "mphip_box_sums"))
    return 1;
  if (box->nx < 1 || box->ny < 1 || box->nz < 1)
    return fail(ctx, "mphip_box_sums: empty grid");
  if (qnt < 0 || qnt >= ctx->nq)
    return fail(ctx, "mphip_box_sums: no such quantity");
  if (nmember < 1 || qnt_member >= ctx->nq || (qnt_member < 0 && nmember != 1))
    return fail(ctx, "mphip_box_sums: bad ensemble members");
  if ((is_meteo_quantity(ctx, qnt) || is_meteo_quantity(ctx, qnt_member)) && flush_meteo(ctx))
    return 1;
  const size_t ncell = (size_t) box->nx * (size_t) box->ny * (size_t) box->nz, ntot = ncell * (size_t) nmember;
  if (ntot >= 0x7fffffffULL)
    return fail(ctx, "too many grid cells for 32-bit cell indices");
  BoxSumArgs B;
  memset(&B, 0, sizeof(B));
  B.G = BoxGrid{ box->lon0, box->lon1, box->lat0, box->lat1, box->z0, box->z1, box->nx, box->ny, box->nz };
  B.t0 = t - 0.5 * ctx->ctl.dt_mod;
  B.t1 = t + 0.5 * ctx->ctl.dt_mod;
  B.qnt = qnt;
  B.qnt_member = qnt_member;
  B.nmember = nmember;
  B.ncell = (int) ncell;
  if (ana_kernel_fn(ctx, nk, kz, kw, &B.K) || reserve(ctx, ctx->d_sums, ntot)
      || reserve(ctx, ctx->d_rec, (size_t) std::max<long long>(ctx->np, 1)))
    return 1;
  int *bad = (int *) ctx->d_ana_flags.p;
  HIPCHK(hipMemsetAsync(bad, 0x7f, sizeof(int), ctx->stream));   // 0x7f7f7f7f: above every index
  hipLaunchKernelGGL(box_member_cell_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, dev_atm(ctx), B, ctx->d_cell.p,
                     ctx->d_rec.p, bad);
  HIPCHK(hipGetLastError());
  int h_bad = 0;
  HIPCHK(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (h_bad != 0x7f7f7f7f)
    return fail(ctx, "Ensemble ID out of range! (particle " + std::to_string(ctx->ip0 + h_bad) + ")");
  const ArrayVals vals = { ctx->d_rec.p };
  if (ordered_cell_sums(ctx, vals, 1, box->nz, ntot, ctx->d_sums.p, (int *) nullptr, (double *) nullptr, true))
    return 1;
  if (run_allreduce(ctx, ctx->d_sums.p, ntot) || reserve(ctx, ctx->h_sums, ntot))
    return 1;
  HIPCHK(hipMemcpyAsync(ctx->h_sums.p, ctx->d_sums.p, ntot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  memcpy(sum, ctx->h_sums.p, ntot * sizeof(double));
  return 0;
}

int mphip_sample_obs(mphip_ctx *ctx, double t0, double t1, int nobs, const double *obs_lon, const double *obs_lat,
                     const double *obs_z, double dx, double dz, int nk, const double *kz, const double *kw, int *count,
                     double *mass) {
  if (!ctx || nobs < 0 || (nobs > 0 && (!obs_lon || !obs_lat || !obs_z || !count)))
    return fail(ctx, "null argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (ana_common(ctx, "mphip_sample_obs"))
    return 1;
  if (nobs == 0)
    return 0;
  const int qnt_m = ctx->ctl.qnt_m >= 0 && ctx->ctl.qnt_m < ctx->nq ? ctx->ctl.qnt_m : -1;
  if (is_meteo_quantity(ctx, qnt_m) && flush_meteo(ctx))
    return 1;
  SampleArgs S;
  memset(&S, 0, sizeof(S));
  S.t0 = t0;
  S.t1 = t1;
  S.reach_lat = dx * 180. / (M_PI * 6367.421);
  S.reach2 = dx * dx;
  S.dz = dz;
  S.nobs = nobs;
  S.qnt_m = qnt_m;
  MarkScan M;
  if (ana_kernel_fn(ctx, nk, kz, kw, &S.K) || reserve(ctx, ctx->d_sums, (size_t) (kObsFields + 2) * (size_t) nobs)
      || ensure_marks(ctx, &M))
    return 1;
  // the observations as the kernel stages them: centre, latitude, pressures of the top and the bottom of the layer
  std::vector<double> h_obs((size_t) kObsFields * (size_t) nobs);
  for (int i = 0; i < nobs; i++) {
    double *o = &h_obs[(size_t) kObsFields * (size_t) i];
    geo2cart_host(obs_lon[i], obs_lat[i], o);
    o[3] = obs_lat[i];
    o[4] = 1013.25 * exp(-(obs_z[i] + dz) / 7.0);
    o[5] = 1013.25 * exp(-(obs_z[i] - dz) / 7.0);
  }
  double *d_obs = ctx->d_sums.p, *d_out = ctx->d_sums.p + (size_t) kObsFields * (size_t) nobs;
  HIPCHK(hipMemcpyAsync(d_obs, h_obs.data(), h_obs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(d_out, 0, 2 * (size_t) nobs * sizeof(double), ctx->stream));
  uint32_t nrec = 0;
  if (ctx->np > 0) {
    const DevAtm a = dev_atm(ctx);
    const int blocks = grid_for(ctx->np);
    hipLaunchKernelGGL(sample_hits_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, a, S, d_obs, ctx->d_marks.p,
                       (const uint32_t *) nullptr, 0, (uint32_t *) nullptr, (double *) nullptr);
    HIPCHK(hipGetLastError());
    // the number of records: every particle's count is at most nobs, so 64 bits hold their sum; the scan works in 32
    HIPCHK(hipMemsetAsync(ctx->d_ana_flags.p + 2, 0, 2 * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(count_total_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream,
                       (const uint32_t *) ctx->d_marks.p, ctx->np, (unsigned long long *) (ctx->d_ana_flags.p + 2));
    if (scan_marks(ctx, M))
      return 1;
    uint32_t h_flags[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(h_flags, ctx->d_ana_flags.p, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const unsigned long long total = ((unsigned long long) h_flags[3] << 32) | h_flags[2];
    if (total > 0x7fffffffULL || total != h_flags[1])
      return fail(ctx, "mphip_sample_obs: more than 2^31 (observation, particle) pairs in one time step");
    nrec = h_flags[1];
    if (nrec > 0) {
      const size_t words32 = 4 * (size_t) nrec;
      HIPCHK(ctx->d_lists.reserve((words32 + 1) / 2));
      if (reserve(ctx, ctx->d_rec, nrec))
        return 1;
      uint32_t *base = (uint32_t *) ctx->d_lists.p;
      uint32_t *keys[2] = { base, base + 2 * (size_t) nrec };
      int *ids[2] = { (int *) (base + (size_t) nrec), (int *) (base + 3 * (size_t) nrec) };
      hipLaunchKernelGGL(sample_hits_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, a, S, d_obs, ctx->d_marks.p,
                         (const uint32_t *) M.chunk_off, M.shift, keys[0], ctx->d_rec.p);
      HIPCHK(hipGetLastError());
      int cur = 0;
      if (radix_passes(ctx, keys, ids, nrec, bits_for((unsigned long long) (nobs - 1)), &cur, nullptr, true))
        return 1;
      hipLaunchKernelGGL(sample_sum_kernel, dim3(grid_for((long long) nobs * 64)), dim3(256), 0, ctx->stream, keys[cur],
                         ids[cur], ctx->d_rec.p, nrec, nobs, d_out);
      HIPCHK(hipGetLastError());
    }
  }
  if (run_allreduce(ctx, d_out, 2 * (size_t) nobs) || reserve(ctx, ctx->h_sums, 2 * (size_t) nobs))
    return 1;
  HIPCHK(hipMemcpyAsync(ctx->h_sums.p, d_out, 2 * (size_t) nobs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < nobs; i++) {
    count[i] = (int) ctx->h_sums.p[(size_t) nobs + (size_t) i];
    if (mass)
      mass[i] = ctx->h_sums.p[i];
  }
  return 0;
}

int mphip_station_hits(mphip_ctx *ctx, double t, double lon, double lat, double r, double stat_t0, double stat_t1,
                       int qnt_stat, int cap, int *nhit, int *index, double *rows) {
  if (!ctx || !nhit || cap < 0 || (cap > 0 && (!index || !rows)))
    return fail(ctx, "null argument");
  HIPCHK(hipSetDevice(ctx->device));
  *nhit = 0;
  if (ana_common(ctx, "mphip_station_hits"))
    return 1;
  if (ctx->comm || ctx->np != ctx->np_total)
    return fail(ctx, "mphip_station_hits: the station output needs all particles in one process");
  if (qnt_stat >= ctx->nq)
    return fail(ctx, "mphip_station_hits: no such quantity");
  if (flush_meteo(ctx))   // (the rows deliver every quantity)
    return 1;
  if (ctx->np == 0)
    return 0;
  StationArgs S;
  memset(&S, 0, sizeof(S));
  S.t0 = t - 0.5 * ctx->ctl.dt_mod;
  S.t1 = t + 0.5 * ctx->ctl.dt_mod;
  S.s0 = stat_t0;
  S.s1 = stat_t1;
  S.reach2 = r * r;
  geo2cart_host(lon, lat, S.centre);
  S.qnt_stat = qnt_stat < 0 ? -1 : qnt_stat;
  MarkScan M;
  if (ensure_marks(ctx, &M) || reserve(ctx, ctx->d_rec, (size_t) ctx->np))
    return 1;
  HIPCHK(ctx->d_slot_of.reserve((size_t) ctx->np));
  const DevAtm a = dev_atm(ctx);
  hipLaunchKernelGGL(station_mark_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, a, S, ctx->d_marks.p,
                     ctx->d_slot_of.p, ctx->d_rec.p);
  HIPCHK(hipGetLastError());
  if (scan_marks(ctx, M))
    return 1;
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, ctx->d_ana_flags.p + 1, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *nhit = (int) total;
  if (total == 0)
    return 0;
  if (total > (uint32_t) cap) {   // the caller comes back with a larger buffer: nothing may have changed
    if (S.qnt_stat >= 0) {
      hipLaunchKernelGGL(station_restore_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, a, S.qnt_stat,
                         (const uint32_t *) ctx->d_marks.p, (const uint32_t *) M.chunk_off, M.shift, (const int *) ctx->d_slot_of.p,
                         (const double *) ctx->d_rec.p);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return 0;
  }
  const size_t width = 5 + (size_t) ctx->nq, words = (size_t) total * width;
  if (reserve(ctx, ctx->d_sums, words) || reserve(ctx, ctx->h_sums, words))
    return 1;
  hipLaunchKernelGGL(station_rows_kernel, dim3(grid_for(ctx->np)), dim3(256), 0, ctx->stream, a, ctx->nq,
                     (const uint32_t *) ctx->d_marks.p, (const uint32_t *) M.chunk_off, M.shift, (const int *) ctx->d_slot_of.p,
                     ctx->d_sums.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ctx->h_sums.p, ctx->d_sums.p, words * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < total; k++) {
    index[k] = (int) ctx->h_sums.p[k * width];
    memcpy(rows + k * (width - 1), ctx->h_sums.p + k * width + 1, (width - 1) * sizeof(double));
  }
  return 0;
}

namespace {

// an enabled range of mphip_select_atm: no NaN bound, lower <= upper
bool select_range_ok(int use, double lo, double hi) {
  return !use || lo <= hi;
}

// One start/stop pair around a stage of mphip_select_atm when that stage is what is being timed (option
// "select_profile_phase": 0 every kernel, 1 mark, 2 scan, 3 list, 4 the row gathers, 5 the copies to the host).
int select_prof(mphip_ctx *ctx, int phase, bool kernel, hipEvent_t *stop) {
  *stop = nullptr;
  if (ctx->select_profile_phase == phase || (ctx->select_profile_phase == 0 && kernel))
    return prof_pair(ctx, ctx->stream, stop);
  return 0;
}

int select_prof_stop(mphip_ctx *ctx, hipEvent_t stop) {
  if (stop)
    HIPCHK(hipEventRecord(stop, ctx->stream));
  return 0;
}

}   // namespace

int mphip_select_atm(mphip_ctx *ctx, const mphip_select_t *sel, long long cap, long long *nsel, int *index, double *time,
                     double *p, double *lon, double *lat, double *const *q) {
  if (!ctx || !sel || !nsel)
    return fail(ctx, "mphip_select_atm: null argument");
  if (!ctx->have_ctl)
    return fail(ctx, "mphip_select_atm: control parameters were not uploaded");
  if (sel->stride < 1)
    return fail(ctx, "mphip_select_atm: stride must be >= 1");
  if (sel->first < 0)
    return fail(ctx, "mphip_select_atm: first must be >= 0");
  if (cap < 0)
    return fail(ctx, "mphip_select_atm: cap must be >= 0");
  if (!select_range_ok(sel->use_time, sel->t0, sel->t1))
    return fail(ctx, "mphip_select_atm: bad time range (a bound is NaN or t0 > t1)");
  if (!select_range_ok(sel->use_z, sel->z0, sel->z1))
    return fail(ctx, "mphip_select_atm: bad height range (a bound is NaN or z0 > z1)");
  if (!select_range_ok(sel->use_lon, sel->lon0, sel->lon1))
    return fail(ctx, "mphip_select_atm: bad longitude range (a bound is NaN or lon0 > lon1)");
  if (!select_range_ok(sel->use_lat, sel->lat0, sel->lat1))
    return fail(ctx, "mphip_select_atm: bad latitude range (a bound is NaN or lat0 > lat1)");
  if (sel->use_near && !(sel->near_r >= 0 && std::isfinite(sel->near_r)))
    return fail(ctx, "mphip_select_atm: near_r must be finite and >= 0");
  if ((sel->use_lon || sel->use_lat || sel->use_near) && ctx->ctl.met_coord_type != 0)
    return fail(ctx, "mphip_select_atm: lon, lat and near need a lat/lon grid (MET_COORD_TYPE 0)");
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))   // (the rows deliver every quantity)
    return 1;
  const long long np = ctx->np;
  const long long last = sel->last < 0 || sel->last >= np ? np - 1 : sel->last;
  if (np == 0 || sel->first > last) {
    *nsel = 0;
    return 0;
  }
  SelectArgs S;
  memset(&S, 0, sizeof(S));
  S.first = (uint32_t) sel->first;
  S.last = (uint32_t) last;
  S.stride = (uint32_t) std::min<long long>(sel->stride, 0x7fffffffLL);   // (np < 2^31: beyond it only `first` is a candidate)
  S.use_time = sel->use_time != 0;
  S.use_z = sel->use_z != 0;
  S.use_lon = sel->use_lon != 0;
  S.use_lat = sel->use_lat != 0;
  S.use_near = sel->use_near != 0;
  S.t0 = sel->t0, S.t1 = sel->t1;
  S.z0 = sel->z0, S.z1 = sel->z1;
  S.lon0 = sel->lon0, S.lon1 = sel->lon1;
  S.lat0 = sel->lat0, S.lat1 = sel->lat1;
  if (S.use_near) {
    S.reach2 = sel->near_r * sel->near_r;
    geo2cart_host(sel->near_lon, sel->near_lat, S.centre);
  }
  MarkScan M;
  if (ensure_marks(ctx, &M))
    return 1;
  HIPCHK(ctx->d_ana_flags.reserve(8));
  HIPCHK(ctx->d_slot_of.reserve((size_t) np));
  const DevAtm a = dev_atm(ctx);
  hipEvent_t stop = nullptr;
  if (select_prof(ctx, 1, true, &stop))
    return 1;
  hipLaunchKernelGGL(select_mark_kernel, dim3(grid_for(np)), dim3(256), 0, ctx->stream, a, S, ctx->d_marks.p, ctx->d_slot_of.p);
  HIPCHK(hipGetLastError());
  if (select_prof_stop(ctx, stop) || select_prof(ctx, 2, true, &stop) || scan_marks(ctx, M) || select_prof_stop(ctx, stop))
    return 1;
  uint32_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, ctx->d_ana_flags.p + 1, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *nsel = (long long) total;
  if (total == 0 || (long long) total > cap)   // (too small a buffer: the count only; the caller comes back with a larger one)
    return 0;
  double *const dst[4] = { time, p, lon, lat };
  int nrows = index ? 1 : 0;
  for (int k = 0; k < 4 + ctx->nq; k++)
    nrows += (k < 4 ? dst[k] : q ? q[k - 4] : nullptr) != nullptr;
  if (nrows == 0)
    return 0;
  // the two lists by rank, then row after row through two device rows: the copy of one overlaps the gather of the next
  const size_t n = total;
  HIPCHK(ctx->d_sel_list.reserve(2 * n));
  HIPCHK(ctx->d_sel_rows.reserve(2 * n));
  int *const sel_slot = ctx->d_sel_list.p, *const sel_index = ctx->d_sel_list.p + n;
  if (select_prof(ctx, 3, true, &stop))
    return 1;
  hipLaunchKernelGGL(select_list_kernel, dim3(grid_for(np)), dim3(256), 0, ctx->stream, np, (const uint32_t *) ctx->d_marks.p,
                     (const uint32_t *) M.chunk_off, M.shift, (const int *) ctx->d_slot_of.p, sel_slot, sel_index);
  HIPCHK(hipGetLastError());
  if (select_prof_stop(ctx, stop))
    return 1;
  // To the caller's arrays: through two page-locked rows of the context and a memcpy that runs beside the next row's
  // gather and copy (the default), or -- option "select_direct" -- straight into the caller's arrays, page-locked in one
  // span under option pin_host_atm as mphip_get_atm has them.
  const bool direct = ctx->select_direct;
  if (direct) {
    const void *all[4 + MPHIP_NQ_MAX] = { time, p, lon, lat };
    for (int iq = 0; iq < ctx->nq; iq++)
      all[4 + iq] = q ? q[iq] : nullptr;
    pin_host_span(ctx, all, 4 + ctx->nq, n * sizeof(double));
  } else {
    HIPCHK(ctx->h_sel_rows.reserve(2 * n));
    for (hipEvent_t &e : ctx->sel_copied)
      if (!e)
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  struct Pending {
    void *to;
    size_t bytes;
  } pending[2] = { { nullptr, 0 }, { nullptr, 0 } };
  int turn = 0;
  auto land = [&](int b) -> int {   // the staged row of buffer b reaches the caller
    if (!pending[b].to)
      return 0;
    HIPCHK(hipEventSynchronize(ctx->sel_copied[b]));
    memcpy(pending[b].to, ctx->h_sel_rows.p + (size_t) b * n, pending[b].bytes);
    pending[b].to = nullptr;
    return 0;
  };
  auto send = [&](const void *d_src, void *to, size_t bytes) -> int {   // a finished device row on its way to `to`
    const int b = turn;
    if (select_prof(ctx, 5, false, &stop))
      return 1;
    if (direct) {
      HIPCHK(hipMemcpyAsync(to, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      HIPCHK(hipMemcpyAsync(ctx->h_sel_rows.p + (size_t) b * n, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipEventRecord(ctx->sel_copied[b], ctx->stream));
      pending[b].to = to;
      pending[b].bytes = bytes;
    }
    if (select_prof_stop(ctx, stop))
      return 1;
    turn ^= 1;
    return direct ? 0 : land(turn);   // (the buffer the next row will use: its copy was queued a whole row ago)
  };
  if (index && send(sel_index, index, n * sizeof(int)))
    return 1;
  for (int k = 0; k < 4 + ctx->nq; k++) {
    double *const to = k < 4 ? dst[k] : q ? q[k - 4] : nullptr;
    if (!to)
      continue;
    double *const row = ctx->d_sel_rows.p + (size_t) turn * n;
    if (select_prof(ctx, 4, true, &stop))
      return 1;
    hipLaunchKernelGGL(select_row_kernel, dim3(grid_for((long long) n)), dim3(256), 0, ctx->stream,
                       (const double *) ctx->d_arr[k].p, (const int *) sel_slot, (long long) n, row);
    HIPCHK(hipGetLastError());
    if (select_prof_stop(ctx, stop) || send(row, to, n * sizeof(double)))
      return 1;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (!direct && (land(0) || land(1)))
    return 1;
  return 0;
}

int mphip_set_radio_decay(mphip_ctx *ctx, int on, const int qnt[MPHIP_NRADIO]) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  if (!qnt && on)
    return fail(ctx, "module_radio_decay: null quantity list");
  RadioQnt r = { { -1, -1, -1, -1, -1, -1 } };
  if (qnt)
    for (int k = 0; k < MPHIP_NRADIO; k++)
      r.q[k] = qnt[k] < 0 ? -1 : qnt[k];
  const std::string why = radio_conflict(ctx->ctl, r.q);
  if (!why.empty())
    return fail(ctx, why);
  if (ctx->rdepo_on) {    // (a module_radio_depo that is on keeps a depositing activity)
    const std::string why_depo = radio_depo_conflict(ctx->ctl, r);
    if (!why_depo.empty())
      return fail(ctx, why_depo);
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (flush_meteo(ctx))   // (a deferred module_meteo belongs to the steps before)
    return 1;
  ctx->radio = r;
  ctx->radio_on = on != 0;
  return 0;
}

int mphip_set_radio_depo(mphip_ctx *ctx, int on, const mphip_box_t *grid) {
  if (ctx && ahead_drop(ctx))
    return 1;
  if (!ctx)
    return 1;
  if (!ctx->have_ctl)
    return fail(ctx, "control parameters were not uploaded");
  if (!grid && on)
    return fail(ctx, "module_radio_depo: null ground grid");
  size_t ntot = 0;
  if (grid) {
    if (grid->nz != 1)
      return fail(ctx, "module_radio_depo: the ground grid has one level (nz = 1)");
    if (grid->nx < 1 || grid->ny < 1 || !(grid->lon0 < grid->lon1) || !(grid->lat0 < grid->lat1))
      return fail(ctx, "module_radio_depo: empty or inverted ground grid");
    ntot = (size_t) grid->nx * (size_t) grid->ny + 1;
    if (ntot >= 0x7fffffffULL)
      return fail(ctx, "module_radio_depo: too many grid cells for 32-bit cell indices");
  }
  if (on) {
    const std::string why = radio_depo_conflict(ctx->ctl, ctx->radio);
    if (!why.empty())
      return fail(ctx, why);
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (grid) {
    const mphip_box_t &g = ctx->rdepo_grid;
    const bool same = ctx->d_rdepo_inv.p && g.nx == grid->nx && g.ny == grid->ny && g.lon0 == grid->lon0 && g.lon1 == grid->lon1
      && g.lat0 == grid->lat0 && g.lat1 == grid->lat1;
    if (!same) {   // a new inventory: zero, no time yet
      HIPCHK(hipStreamSynchronize(ctx->stream));
      ctx->rdepo_ntot = 0;
      HIPCHK(ctx->d_rdepo_inv.resize(2 * (size_t) MPHIP_NRADIO * ntot));
      HIPCHK(hipMemsetAsync(ctx->d_rdepo_inv.p, 0, 2 * (size_t) MPHIP_NRADIO * ntot * sizeof(double), ctx->stream));
      ctx->rdepo_grid = *grid;
      ctx->rdepo_ntot = ntot;
      ctx->rdepo_have_t = false;
      ctx->rdepo_t = 0;
    }
  }
  ctx->rdepo_on = on != 0;
  return 0;
}

int mphip_get_radio_depo(mphip_ctx *ctx, double *t_inv, double *wet, double *dry) {
  if (!ctx)
    return 1;
  if (!ctx->d_rdepo_inv.p)
    return fail(ctx, "mphip_get_radio_depo: no inventory (mphip_set_radio_depo has not been called)");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t plane = (size_t) MPHIP_NRADIO * ctx->rdepo_ntot, total = 2 * plane;
  // this rank's part, summed over the ranks in a copy (the inventory itself stays this rank's)
  if (reserve(ctx, ctx->d_sums, total) || reserve(ctx, ctx->h_sums, total))
    return 1;
  HIPCHK(hipMemcpyAsync(ctx->d_sums.p, ctx->d_rdepo_inv.p, total * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (run_allreduce(ctx, ctx->d_sums.p, total))
    return 1;
  HIPCHK(hipMemcpyAsync(ctx->h_sums.p, ctx->d_sums.p, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (t_inv)
    *t_inv = ctx->rdepo_have_t ? ctx->rdepo_t : NAN;
  if (wet)
    memcpy(wet, ctx->h_sums.p, plane * sizeof(double));
  if (dry)
    memcpy(dry, ctx->h_sums.p + plane, plane * sizeof(double));
  return 0;
}

int mphip_set_grid_kernel(mphip_ctx *ctx, int nk, const double *kz, const double *kw) {
  if (!ctx)
    return 1;
  if (nk < 0 || nk > 1024 || (nk >= 2 && (!kz || !kw)))
    return fail(ctx, "bad kernel function");
  for (int k = 1; k < nk; k++)
    if (kz[k] < kz[k - 1])
      return fail(ctx, "height levels of the kernel function must be ascending");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx->d_grid_kernel.resize(nk >= 2 ? 2 * (size_t) nk : 0));
  ctx->grid_nk = nk >= 2 ? nk : 0;
  if (ctx->grid_nk) {
    HIPCHK(hipMemcpy(ctx->d_grid_kernel.p, kz, (size_t) nk * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->d_grid_kernel.p + nk, kw, (size_t) nk * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
}

int mphip_set_allreduce(mphip_ctx *ctx, mphip_allreduce_fn fn, void *user) {
  if (!ctx)
    return 1;
  ctx->allreduce = fn;
  ctx->allreduce_user = user;
  return 0;
}

int mphip_comm_unique_id(void *id128) {
  if (!id128)
    return 1;
  Rccl &R = rccl();
  if (!R.ok) {
    fprintf(stderr, "mptrac_hip: %s\n", R.why.c_str());
    return 2;
  }
  Rccl::UniqueId id;
  StdoutToStderr quiet;
  if (R.GetUniqueId(&id) != 0)
    return 3;
  memcpy(id128, &id, sizeof(id));
  return 0;
}

int mphip_comm_init(mphip_ctx *ctx, int nranks, int rank, const void *id128) {
  if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(ctx, "bad communicator arguments");
  Rccl &R = rccl();
  if (!R.ok)
    return fail(ctx, R.why);
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->comm) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    RCCLCHK(R.CommDestroy(ctx->comm));
    ctx->comm = nullptr;
  }
  Rccl::UniqueId id;
  memcpy(&id, id128, sizeof(id));
  StdoutToStderr quiet;
  RCCLCHK(R.CommInitRank(&ctx->comm, nranks, id, rank));
  ctx->comm_ranks = nranks;
  ctx->comm_rank = rank;
  return 0;
}

int mphip_comm_destroy(mphip_ctx *ctx) {
  if (!ctx)
    return 1;
  if (ctx->comm) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    RCCLCHK(rccl().CommDestroy(ctx->comm));
    ctx->comm = nullptr;
  }
  ctx->comm_ranks = 1;
  ctx->comm_rank = 0;
  return 0;
}

int mphip_comm_query(mphip_ctx *ctx, int *nranks, int *rank) {
  if (!ctx || !nranks || !rank)
    return 1;
  *nranks = 0;
  *rank = 0;
  if (!ctx->comm)
    return 0;
  Rccl &R = rccl();
  RCCLCHK(R.CommCount(ctx->comm, nranks));
  RCCLCHK(R.CommUserRank(ctx->comm, rank));
  return 0;
}

namespace {

// mphip_set_option (documented in include/mptrac_hip.h) as a table: the name, the member it sets, which values are
// accepted, the refusal, and for the few options with a side effect what runs before the store
enum OptKind {
  kFlag,          // value != 0
  kRange,         // (int) value; refused if value < lo or value > hi
  kZeroOrRange,   // (int) value; 0, or within [lo, hi]
  kWhole          // one of the integers lo ... hi
};

struct Option {
  const char *name;
  bool mphip_ctx::*flag;     // kFlag
  int mphip_ctx::*number;    // the other kinds
  OptKind kind;
  double lo, hi;
  const char *refusal;
  int (*before)(mphip_ctx *, double);
};

typedef int (*OptHook)(mphip_ctx *, double);

constexpr Option flag(const char *name, bool mphip_ctx::*member, OptHook before = nullptr) {
  return Option{ name, member, nullptr, kFlag, 0, 0, nullptr, before };
}

constexpr Option number(const char *name, int mphip_ctx::*member, OptKind kind, double lo, double hi, const char *refusal,
                        OptHook before = nullptr) {
  return Option{ name, nullptr, member, kind, lo, hi, refusal, before };
}

int flush_if_switched_off(mphip_ctx *ctx, double value) {
  return value == 0 ? flush_meteo(ctx) : 0;
}

int drop_sort_ahead(mphip_ctx *ctx, double) {
  return ahead_drop(ctx);
}

int resort_next_step(mphip_ctx *ctx, double) {
  ctx->steps_since_resort = 1 << 30;
  return 0;
}

const char *const kStepBlocksRefusal = "step_blocks must be in 8 ... 1048576";

const Option kOptions[] = {
  number("locality_sort_interval", &mphip_ctx::locality_interval, kRange, 0, HUGE_VAL, "locality_sort_interval must be >= 0"),
  number("step_blocks", &mphip_ctx::step_blocks, kRange, 8, 1048576, kStepBlocksRefusal),
  number("step_blocks_multi", &mphip_ctx::step_blocks_multi, kRange, 8, 1048576, kStepBlocksRefusal),
  flag("fuse_sort", &mphip_ctx::fuse_sort),                   // 0: module_sort re-orders every array in its own pass
  // 0: run module_meteo inside every time step that schedules it
  flag("lazy_meteo", &mphip_ctx::lazy_meteo, flush_if_switched_off),
  flag("pin_host_atm", &mphip_ctx::pin_host_atm),             // page-lock the arrays handed to mphip_update_atm / mphip_get_atm
  // mphip_run_timesteps: most steps per launch, 0 = one launch per step
  number("multi_step", &mphip_ctx::multi_step, kRange, 0, 4096, "multi_step must be in 0 ... 4096"),
  flag("fold_resort", &mphip_ctx::fold_resort),               // 0: the locality re-sort always gathers in a pass of its own
  flag("turb_strat", &mphip_ctx::turb_strat),                 // 0: module_diff_turb never takes its short path above the tropopause
  flag("fuse_sort_quantities", &mphip_ctx::fuse_quantities),  // 0: module_sort moves the quantity arrays in a pass of its own
  flag("perm_records", &mphip_ctx::perm_records),
  flag("big_grid", &mphip_ctx::big_grid),
  number("derive_profile_phase", &mphip_ctx::derive_profile_phase, kWhole, 0, 6,
         "derive_profile_phase must be 0 (kernels), 1 (uploads), 2 (downloads), 3 (the weight table of "
         "mphip_detrend_met) or 4, 5, 6 (the extremes, their reduction, the quantisation of mphip_pack_met)"),
  flag("xcd_map", &mphip_ctx::xcd_map),
  // the step kernel's chunk queues: 0 = the static partition, 1 = launches of 16 chunks per resident wave or more, 2 = all
  number("step_queue", &mphip_ctx::step_queue, kWhole, 0, 2, "step_queue must be 0, 1 or 2"),
  flag("generic_kernel", &mphip_ctx::force_generic),          // tuning aid: never pick a specialised instantiation
  number("sort_bits", &mphip_ctx::sort_bits, kZeroOrRange, 8, kRadixMaxBits, "sort_bits must be 0 (automatic), 8, 9 or 10"),
  flag("mix_exchange_levels", &mphip_ctx::mix_exchange_levels),   // 0: the exchange of a mixing step covers the whole grid
  // cells of the LDS wind tile for runs of pure trajectory steps (24 bytes each; 0: off)
  number("lds_tile", &mphip_ctx::lds_tile, kZeroOrRange, 64, 2400, "lds_tile must be 0 or 64 ... 2400 cells"),
  flag("ahead_priority", &mphip_ctx::ahead_priority),         // (before the first sort ahead: the stream is created then)
  flag("emit_keys", &mphip_ctx::emit_keys),                   // 0: the keys of the sort ahead come from a kernel of their own
  flag("sort_repair", &mphip_ctx::sort_repair),               // 0: the module_sort that runs ahead always sorts from scratch
  flag("compact_depo", &mphip_ctx::compact_depo),             // 0: deposition-only launches run the tail of the fused kernel
  flag("ahead_box", &mphip_ctx::ahead_box),                   // tuning aid
  flag("sort_ahead", &mphip_ctx::sort_ahead, drop_sort_ahead),   // 0: module_sort runs when mphip_run_timestep reaches it
  // tests: force one of the ordered-sum algorithms (0: choose by crowding)
  number("sum_path", &mphip_ctx::sum_path, kWhole, 0, 2, "sum_path must be 0, 1 or 2"),
  // 1 (default): cell sums of module_mixing / the gridded output add in the reference's serial order;
  // 0: floating-point atomics (order of arrival)
  number("deterministic_sums", &mphip_ctx::deterministic_sums, kWhole, 0, 1, "deterministic_sums must be 0 or 1"),
  flag("grid_records", &mphip_ctx::grid_records),             // tuning / tests: 0 = gather the gridded sums' values from the arrays
  number("chain_blocks", &mphip_ctx::chain_blocks, kRange, -HUGE_VAL, HUGE_VAL, nullptr),   // (any value)
  flag("locality_zorder", &mphip_ctx::locality_zorder, resort_next_step),
  number("locality_tile", &mphip_ctx::locality_tile, kRange, 0, 64, "locality_tile must be in 0 ... 64", resort_next_step),
  // points per launch of mphip_intpol_met
  number("intpol_chunk", &mphip_ctx::intpol_chunk, kRange, 64, 1 << 24, "intpol_chunk must be in 64 ... 16777216"),
  // mphip_select_atm: 1 = rows are copied straight into the caller's arrays (page-locked under pin_host_atm)
  flag("select_direct", &mphip_ctx::select_direct),
  number("select_profile_phase", &mphip_ctx::select_profile_phase, kWhole, 0, 5,
         "select_profile_phase must be 0 (kernels), 1 (mark), 2 (scan), 3 (list), 4 (row gathers) or 5 (copies)"),
};

}   // namespace

int mphip_set_option(mphip_ctx *ctx, const char *name, double value) {
  if (!ctx || !name)
    return 1;
  for (const Option &o : kOptions) {
    if (strcmp(name, o.name) != 0)
      continue;
    const bool inside = value >= o.lo && value <= o.hi;
    if ((o.kind == kRange && (value < o.lo || value > o.hi)) || (o.kind == kZeroOrRange && !(value == 0 || inside))
        || (o.kind == kWhole && !(inside && value == std::floor(value))))
      return fail(ctx, o.refusal);
    if (o.before && o.before(ctx, value))
      return 1;
    if (o.kind == kFlag)
      ctx->*o.flag = value != 0;
    else
      ctx->*o.number = (int) value;
    return 0;
  }
  return fail(ctx, std::string("unknown option ") + name);
}

int mphip_get_shortcuts(mphip_ctx *ctx, double bounds[4]) {
  if (!ctx || !bounds)
    return fail(ctx, "null argument");
  if (!ctx->slot[0].valid || !ctx->slot[1].valid)
    return fail(ctx, "mphip_get_shortcuts: needs both meteo snapshots");
  const DevMet M = dev_met(ctx);
  bounds[0] = M.ps_skip;
  bounds[1] = M.pct_skip;
  bounds[2] = M.turb_skip;
  bounds[3] = M.conv_skip;
  return 0;
}

int mphip_synchronize(mphip_ctx *ctx) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_profile_begin(mphip_ctx *ctx) {
  if (!ctx)
    return 1;
  ctx->prof = true;
  ctx->ev_used = 0;
  return 0;
}

int mphip_profile_end(mphip_ctx *ctx, long long *launches, double *kernel_ms) {
  if (!ctx)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  double total = 0;
  for (size_t k = 0; k + 1 < ctx->ev_used; k += 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev[k], ctx->ev[k + 1]));
    total += ms;
  }
  if (launches)
    *launches = (long long) (ctx->ev_used / 2);
  if (kernel_ms)
    *kernel_ms = total;
  ctx->prof = false;
  ctx->ev_used = 0;
  return 0;
}

int mphip_test_sincosf(mphip_ctx *ctx, uint32_t bits_first, uint32_t count, float *cos_out, float *sin_out) {
  if (!ctx || !cos_out || !sin_out)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<float> dc, ds;
  HIPCHK(dc.resize(count));
  HIPCHK(ds.resize(count));
  hipLaunchKernelGGL(test_sincosf_kernel, dim3(grid_for(count)), dim3(256), 0, ctx->stream, bits_first, count, dc.p, ds.p);
  HIPCHK(hipMemcpyAsync(cos_out, dc.p, (size_t) count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(sin_out, ds.p, (size_t) count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_test_libm(mphip_ctx *ctx, int op, const double *x, const double *y, long long n, double *out) {
  if (!ctx || !x || !out || n < 0 || ((op & 15) == 2 && !y) || (op & ~31) || (op & 15) > 7)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t count = (size_t) std::max<long long>(n, 1);
  DevBuf<double> dx, dy, dout;
  HIPCHK(dx.resize(count));
  HIPCHK(dout.resize(count));
  HIPCHK(hipMemcpyAsync(dx.p, x, (size_t) n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((op & 15) == 2) {
    HIPCHK(dy.resize(count));
    HIPCHK(hipMemcpyAsync(dy.p, y, (size_t) n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(test_libm_kernel, dim3(grid_for(std::max<long long>(n, 1))), dim3(256), 0, ctx->stream, op, dx.p, dy.p, n,
                     dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int mphip_test_piece(mphip_ctx *ctx, int piece, int reps, double *checksum) {
  if (!ctx || !ctx->have_ctl || ctx->np == 0)
    return fail(ctx, "mphip_test_piece needs control parameters and particles");
  HIPCHK(hipSetDevice(ctx->device));
  if (ensure_packed(ctx))
    return 1;
  if (!ctx->have_clim)
    return fail(ctx, "climatological tropopause data were not uploaded");
  StepParams S;
  memset(&S.emit, 0, sizeof(S.emit));
  S.depo_busy = nullptr;
  S.ctl = ctx->ctl;
  S.met = dev_met(ctx);
  S.atm = dev_atm(ctx);
  S.clim = ctx->d_clim.p;
  S.tracers = ctx->d_tracers.p;
  S.t = 0;
  S.mask = 0;
  const BlockGeom geom = block_geom(ctx->np, ctx->step_blocks);
  const int nb = geom.nblocks_logical;
  S.nblocks_logical = nb;
  S.per_block = geom.per_block;
  S.xcd_map = ctx->xcd_map;
  S.ctr_turb = 1000;
  S.ctr_meso = 5000;
  S.ctr_conv = 9000;
  S.ctr_pbl = 0;
  S.queue = nullptr;
  S.queue_n = S.queue_chunks = S.queue_waves = 0;
  if (piece == 22) {   // (diff_meso_fast reads the table)
    if (!lean32_ok(ctx))
      return fail(ctx, "mphip_test_piece: piece 22 needs a grid the lean kernels with 32-bit offsets run on");
    if (ensure_meso_table(ctx))
      return 1;
    S.met.meso = ctx->pk.meso.p;
  }
  DevBuf<double> out;
  HIPCHK(out.resize((size_t) ctx->np));
  double *const d = out.p;
  const size_t lds = axes_lds_bytes(ctx) + sizeof(DevClim) + (size_t) kLibmLogExpDoubles * sizeof(double);
  switch (piece) {
#define PIECE_CASE(K)                                                                                  \
  case K:                                                                                              \
    hipLaunchKernelGGL(piece_kernel<K>, dim3(nb), dim3(256), lds, ctx->stream, S, reps, d);            \
    break;
#ifdef MPHIP_QUICK
    PIECE_CASE(0)
#else
    PIECE_CASE(0) PIECE_CASE(1) PIECE_CASE(2) PIECE_CASE(3) PIECE_CASE(4) PIECE_CASE(5) PIECE_CASE(6) PIECE_CASE(7)
    PIECE_CASE(8) PIECE_CASE(9) PIECE_CASE(10) PIECE_CASE(11) PIECE_CASE(12) PIECE_CASE(13) PIECE_CASE(14)
    PIECE_CASE(15) PIECE_CASE(16) PIECE_CASE(17) PIECE_CASE(18) PIECE_CASE(19) PIECE_CASE(20) PIECE_CASE(21)
    PIECE_CASE(22) PIECE_CASE(23) PIECE_CASE(24) PIECE_CASE(25) PIECE_CASE(26)
#endif
#undef PIECE_CASE
  default:
    return fail(ctx, "unknown piece");
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (checksum) {
    std::vector<double> h((size_t) std::min<long long>(ctx->np, 1024));
    HIPCHK(hipMemcpy(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    double sum = 0;
    for (double v : h)
      sum += v;
    *checksum = sum;
  }
  return 0;
}

int mphip_test_meso_table(mphip_ctx *ctx, float *out, size_t cells) {
  if (!ctx || !out)
    return fail(ctx, "bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  if (ensure_packed(ctx))
    return 1;
  const size_t nx = (size_t) ctx->nx - 1, ny = (size_t) ctx->ny - 1, np = (size_t) ctx->npl - 1;
  if (cells != nx * ny * np)
    return fail(ctx, "mphip_test_meso_table: `cells` must be (nx - 1) (ny - 1) (np - 1)");
  if (!lean32_ok(ctx))
    return fail(ctx, "mphip_test_meso_table: no table on this grid");
  if (ensure_meso_table(ctx))
    return 1;
  std::vector<float> h(meso_table_floats(ctx));
  HIPCHK(hipMemcpyAsync(h.data(), ctx->pk.meso.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t nty = (size_t) (ctx->ny + 2) / 4;
  for (size_t ix = 0; ix < nx; ix++)
    for (size_t iy = 0; iy < ny; iy++)
      for (size_t ip = 0; ip < np; ip++) {
        const size_t o = ((((ix >> 2) * nty + (iy >> 2)) * np + ip) << 4) + ((ix & 3) << 2) + (iy & 3);
        for (int k = 0; k < 3; k++)
          out[3 * ((ix * ny + iy) * np + ip) + k] = h[3 * o + k];
      }
  return 0;
}

int mphip_test_rng(mphip_ctx *ctx, uint64_t ctr, long long n, int method, double *out) {
  if (!ctx || !out || n < 0)
    return 1;
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<double> d;
  HIPCHK(d.resize((size_t) std::max<long long>(n, 1)));
  hipLaunchKernelGGL(test_rng_kernel, dim3(grid_for(std::max<long long>(n, 1))), dim3(256), 0, ctx->stream, ctr, n,
                     method, d.p);
  HIPCHK(hipMemcpyAsync(out, d.p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

}   // extern "C"

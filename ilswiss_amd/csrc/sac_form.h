// sac_form.h — the form a SAC gradient step takes, as a value, and the one place that decides it.
// Host-only and free of HIP: a host harness compiles it as it stands (tests/harness/sac_form_host.cpp).
#pragma once
#include <functional>

struct ilsx_replay;
struct SacCollector;

// what the stage functions of ilsx_sac.hip do with the descriptors they build: launch them; (phase steps) put the two descriptor blocks into
// the agent's constant-memory slots and launch nothing; (phase steps) only hold the blocks against what the phase kernels are compiled for
enum SacFormMode { SAC_FORM_LAUNCH = 0, SAC_FORM_UPLOAD = 1, SAC_FORM_CHECK = 2 };

struct SacStepForm {
  ilsx_replay* ring = nullptr;   // the ring the step's rows come from (column-split path: drawn inside the first launch), or null: a staged batch
  SacCollector* col = nullptr;   // grouped build: the launch sites hand their descriptors to this list instead of launching
  bool fuse = false;             // Adam (+ Polyak) inside the weight-gradient epilogue, the tail as one launch
  bool defer_tail = false;       // the tail rides in the next step's first launch (the window's decision: sac_defer_begin)
  bool phase = false;            // the merged phase kernels
  bool own_rows = false;         // phase A: the target critics on grid rows of their own
  int mode = SAC_FORM_LAUNCH;
  bool operator==(const SacStepForm& o) const {
    return ring == o.ring && col == o.col && fuse == o.fuse && defer_tail == o.defer_tail && phase == o.phase && own_rows == o.own_rows && mode == o.mode;
  }
  bool operator!=(const SacStepForm& o) const { return !(*this == o); }
};

// What the decision rests on.  The callables need the device or a dry pass: asked last, in this order, only when every term before them holds.
struct SacFormInputs {
  int cs = 1;                  // column-split factor (1: generic kernels)
  bool wide_l0 = false;        // two-launch forward for wide inputs (h0scr)
  bool collecting = false;     // the step is being collected for a grouped build
  bool phase_broken = false;   // a phase window was rolled back once: the agent stays on one launch per stage
  int xcd_shift = 0;           // ILSX_XCD_SHIFT of the context
  bool split = false;          // gradient all-reduce between backward and update
  bool no_phase = false, no_fuse = false;   // ILSX_NO_PHASE (read per call), ILSX_NO_FUSE
  std::function<bool()> phase_fits;       // every workgroup of a phase launch of this batch is resident at once
  std::function<bool()> static_heads;     // the agent's descriptor blocks are what the phase kernels are compiled for (a dry pass, once per agent)
  std::function<bool()> phase_own_rows;   // phase A's mapping for this batch
};

// May a window of steps on this batch run on the merged phase kernels?  Each term once, the cheap ones first (their reasons: DESIGN §30).
inline bool sac_window_may_phase(const SacFormInputs& in) {
  return !in.no_phase && !in.phase_broken && in.cs > 1 && !in.wide_l0 && !in.collecting && in.xcd_shift == 0 && in.phase_fits() && in.static_heads();
}
// May this step?  The window's answer and the window's deferred tail (a split run defers its tail only for the phase kernels).
inline bool sac_step_may_phase(const SacFormInputs& in, bool window_defer_tail) { return window_defer_tail && sac_window_may_phase(in); }

// The form of a step on rows from `ring` (null: staged) inside a window that decided `window_defer_tail` (false: no window open).
inline SacStepForm sac_step_form(const SacFormInputs& in, bool window_defer_tail, ilsx_replay* ring, SacCollector* col = nullptr) {
  SacStepForm f;
  f.ring = ring; f.col = col; f.defer_tail = window_defer_tail;
  f.fuse = !in.no_fuse && !in.split;
  f.phase = sac_step_may_phase(in, window_defer_tail);
  f.own_rows = f.phase && in.phase_own_rows();
  return f;
}

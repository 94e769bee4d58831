// switches.h — the one place libilsx.so reads its environment: one row per variable (INTEGRATION §6 is the same table in prose,
// tests/test_switch_table.py holds the two together), one typed accessor per row: sw::ILSX_NO_PHASE(), sw::ILSX_DW_TILE(), ...
// Host-only and free of HIP (tests/harness/sac_form_host.cpp compiles it against a stub environment).
#pragma once
#include <cstdlib>

#ifndef ILSX_SWITCH_ENV
#define ILSX_SWITCH_ENV(name) std::getenv(name)
#endif

// Parse rules (rule, C++ type, value):
//   PRESENT  bool  set to anything, the empty string included
//   UNLESS0  bool  on by default; off when set to something atoi() reads as 0 ("0", "", "off")
//   INT      int   atoi() of the value; the row's default when unset
// Lifetimes — when the accessor's value is taken:
//   PROCESS  once per process, at the accessor's first call, wherever that is; later changes of the variable are not seen
//   CONTEXT  at ilsx_ctx_create, copied into the context
//   OBJECT   when the object is created (a group: when its tables are built), kept on the object
//   CALL     at every call of the accessor: tests and A/B tools switch these inside one process
//     name                       rule     default lifetime  meaning
#define ILSX_SWITCHES(X) \
  X(ILSX_NO_PHASE,               PRESENT, 0,  CALL,    "SAC step on one launch per stage instead of the merged phase kernels") \
  X(ILSX_PHASE_OWN_ROWS,         UNLESS0, 1,  CALL,    "0: phase A runs the target critics on the policy rows' workgroups, not on rows of their own") \
  X(ILSX_PHASE_VERBOSE,          PRESENT, 0,  CALL,    "one line on stderr when a phase window is rolled back") \
  X(ILSX_PHASE_CT,               UNLESS0, 1,  PROCESS, "0: phase descriptor blocks in the kernel arguments, not in the constant-memory tables") \
  X(ILSX_PHASE_CT_TRACE,         PRESENT, 0,  PROCESS, "print which form every phase A launch took") \
  X(ILSX_PHASE_CT_NO_REPRIME,    PRESENT, 0,  PROCESS, "test aid: replay a cached step graph without re-priming the constant-memory slots") \
  X(ILSX_NO_GRAPH,               PRESENT, 0,  PROCESS, "train_from_replay launches directly instead of replaying a captured graph") \
  X(ILSX_NO_DEFER_TAIL,          PRESENT, 0,  PROCESS, "the alpha-update tail as a launch of its own") \
  X(ILSX_NO_FUSE,                PRESENT, 0,  PROCESS, "Adam / Polyak as launches of their own") \
  X(ILSX_NO_SPLIT,               PRESENT, 0,  OBJECT,  "the generic MLP kernels instead of the column-split ones") \
  X(ILSX_L0_SPLIT_KP,            INT,     65, OBJECT,  "padded input width from which the column-split forward runs layer 0 in a launch of its own") \
  X(ILSX_ADVIRL_NO_WINDOW,       PRESENT, 0,  PROCESS, "every SAC step of ilsx_advirl_train with its own tail on one launch per stage") \
  X(ILSX_SPLIT_FORCE,            PRESENT, 0,  CALL,    "tests: the split-run code path on a one-rank communicator") \
  X(ILSX_SPLIT_GRAPH,            PRESENT, 0,  PROCESS, "split runs capture the whole step, collectives included") \
  X(ILSX_SPLIT_NO_PHASE,         PRESENT, 0,  CALL,    "a split run keeps one launch per stage") \
  X(ILSX_SPLIT_PHASE,            PRESENT, 0,  CALL,    "a split run of more than one rank may take the phase kernels (the ranks vote per window)") \
  X(ILSX_DW_TILE,                INT,     0,  CALL,    "weight-gradient output tile as NH KT digits (24, 12, 11); 0: by size") \
  X(ILSX_DW_TILE_GRP,            INT,     0,  CALL,    "the same for the grouped weight-gradient launch (read per group build)") \
  X(ILSX_DW_GRP_LOW,             INT,     -1, CALL,    "0 / 1: pin the grouped weight-gradient tile's register instance; negative: by launch size") \
  X(ILSX_DW_BIG,                 INT,     1,  PROCESS, "0: weight gradients of batches >= 4096 rows on the tile kernel instead of k_dw_big") \
  X(ILSX_GRP_CONST,              UNLESS0, 1,  CALL,    "0: grouped descriptor records from the device-memory tables only (read per group build)") \
  X(ILSX_GRP_LATE,               INT,     -1, OBJECT,  "0 / 1: pin the late-weights shape of grouped forward / backward launches; negative: by launch size") \
  X(ILSX_ROLLOUT_NO_GROUP,       PRESENT, 0,  PROCESS, "lock-step rollouts of grouped runs as one launch per run and stage") \
  X(ILSX_REPLAY_NT,              UNLESS0, 1,  PROCESS, "0: k_replay_sample_many with ordinary instead of non-temporal output stores") \
  X(ILSX_XCD_SHIFT,              INT,     0,  CONTEXT, "column-split and weight-gradient launches use every 2^k-th workgroup slot only") \
  X(ILSX_RT,                     INT,     1,  CONTEXT, "16-row tiles a workgroup of the column-split forward walks, single launches") \
  X(ILSX_RT_GROUPED,             INT,     1,  CONTEXT, "the same for grouped launches")

namespace sw {
typedef bool T_PRESENT; typedef bool T_UNLESS0; typedef int T_INT;
inline bool parse_PRESENT(const char* e, int) { return e != nullptr; }
inline bool parse_UNLESS0(const char* e, int) { return !e || std::atoi(e) != 0; }
inline int parse_INT(const char* e, int dflt) { return e ? std::atoi(e) : dflt; }
// a PROCESS accessor keeps its first answer (one function-local static per accessor, shared by every file that includes this header);
// the other lifetimes read now, and it is the caller that keeps the value where the lifetime says
#define ILSX_SW_TAKE_PROCESS(expr) static const auto v = (expr); return v
#define ILSX_SW_TAKE_CONTEXT(expr) return (expr)
#define ILSX_SW_TAKE_OBJECT(expr) return (expr)
#define ILSX_SW_TAKE_CALL(expr) return (expr)
#define ILSX_SW_ACCESSOR(name, rule, dflt, life, meaning) \
  inline T_##rule name() { ILSX_SW_TAKE_##life(parse_##rule(ILSX_SWITCH_ENV(#name), dflt)); }
ILSX_SWITCHES(ILSX_SW_ACCESSOR)
#undef ILSX_SW_ACCESSOR
}  // namespace sw

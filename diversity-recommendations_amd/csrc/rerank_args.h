// Host-side argument checks shared by dr_mmr_rerank, dr_dpp_rerank,
// dr_calibrated_rerank and dr_xquad_rerank: each condition, code and message exists once, and an
// entry point is a short sequence of these calls. A check returns DR_OK, or an
// error code with dr_last_error() = "<fn>: <message>". Where the entry points
// answer differently today they keep their answer (pinned by
// tests/test_rerank_args_host.py): by a CandidateRules each, or by the order
// in which they make the calls.
#pragma once

#include "common.h"

// return what a check_*() below answers unless it is DR_OK
#define DR_CHECK_RC(call)                   \
  do {                                      \
    if (const int rc_ = (call)) return rc_; \
  } while (0)

namespace dr {

constexpr int kRerankMaxC = 1024;  // candidates per user of every re-rank kernel

struct CandidateRules {
  bool any_n_users;         // n_users is not checked
  bool wide_c_unsupported;  // C > 1024 is DR_EUNSUPPORTED, C < 1 a message of its own
  int max_k;                // a bound on k_out besides C
};
constexpr CandidateRules kMmrArgs{true, false, kRerankMaxC};
constexpr CandidateRules kDppArgs{false, false, 128};
constexpr CandidateRules kCalibratedArgs{false, true, kRerankMaxC};
constexpr CandidateRules kXquadArgs{false, true, kRerankMaxC};  // answers like kCalibratedArgs

inline int arg_error(const char* fn, int code, const std::string& msg) {
  set_error(std::string(fn) + ": " + msg);
  return code;
}

// The candidate lists [n_users, C], the number of picks and the trade-off.
inline int check_candidates(const char* fn, int64_t n_users, int C, int k_out, float lambda,
                            const CandidateRules& rules) {
  if (!rules.any_n_users && n_users < 0) return arg_error(fn, DR_EINVAL, "n_users must be >= 0");
  if (rules.wide_c_unsupported) {
    if (C > kRerankMaxC) return arg_error(fn, DR_EUNSUPPORTED, "C must be <= 1024");
    if (C < 1) return arg_error(fn, DR_EINVAL, "C must be >= 1");
  } else if (C < 1 || C > kRerankMaxC) {
    return arg_error(fn, DR_EINVAL, "C must be in [1, 1024]");
  }
  if (k_out < 1 || k_out > C || k_out > rules.max_k)
    return arg_error(fn, DR_EINVAL,
                     rules.max_k < kRerankMaxC
                         ? "k_out must be in [1, min(C, " + std::to_string(rules.max_k) + ")]"
                         : std::string("k_out must be in [1, C]"));
  if (!(lambda >= 0.f && lambda <= 1.f))  // NaN fails
    return arg_error(fn, DR_EINVAL, "lambda must be in [0, 1]");
  return DR_OK;
}

// The fp32 item-aspect matrix [n_items, G] of dr_xquad_rerank, dr_aspect_profile
// and dr_aspect_coverage, and the cells of a user's C x G block in LDS (the
// re-rank alone; the other two pass C = 0).
inline int check_aspects(const char* fn, int64_t n_items, int G, int C = 0) {
  if (G > DR_XQUAD_MAX_ASPECTS) return arg_error(fn, DR_EUNSUPPORTED, "G must be <= 64");
  if (G < 1 || n_items < 0 || n_items >= 0x7fffffffLL)
    return arg_error(fn, DR_EINVAL, "G must be >= 1 and n_items in [0, 2^31)");
  if ((int64_t)C * G > DR_XQUAD_MAX_CELLS)
    return arg_error(fn, DR_EUNSUPPORTED, "C * G must be <= 32768");
  return DR_OK;
}
// once there are users, rows or lists: no aspect row an id could name
inline int check_aspects_filled(const char* fn, int64_t n_items) {
  return n_items == 0 ? arg_error(fn, DR_EINVAL, "empty aspect matrix") : DR_OK;
}

// The bf16 item table [n_items, d], in three steps: the entry points return
// for n_users == 0, and look at their pointers, between different ones.
inline int check_item_rows(const char* fn, int64_t n_items) {
  if (n_items < 0 || n_items >= 0x7fffffffLL)
    return arg_error(fn, DR_EINVAL, "n_items must be in [0, 2^31)");
  return DR_OK;
}
inline int check_item_width(const char* fn, int d) {  // the widths with a kernel instance
  if (d != 64 && d != 128) return arg_error(fn, DR_EUNSUPPORTED, "d must be 64 or 128");
  return DR_OK;
}
// once there are users: no row a candidate could name (the kernels read row 0 for empty slots)
inline int check_item_table_filled(const char* fn, int64_t n_items) {
  return n_items == 0 ? arg_error(fn, DR_EINVAL, "empty item table") : DR_OK;
}

}  // namespace dr

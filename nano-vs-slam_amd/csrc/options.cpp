// The three readers of kOptions (options.h) and the launchers' Tuning.
#include "options.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "api_common.h"

namespace kp2d {

Options::Options() {
  for (const OptionRow& r : kOptions) this->*r.field = (int)r.def;
  lanes_default = lanes;
}

void options_from_env(Options& o, const char* (*get)(const char*)) {
  for (const OptionRow& r : kOptions) {
    const char* e = r.var ? get(r.var) : nullptr;
    if (!e) continue;
    int& f = o.*r.field;
    const long v = atol(e), top = std::min(v, r.max);
    switch (r.env) {
      case Env::none: break;
      case Env::off: if (e[0] == '0') f = 0; break;
      case Env::clamp: f = (int)std::max(r.min, std::min(r.max, (long)atoi(e))); break;
      case Env::lanes: f = o.lanes_default = (int)std::max(1L, std::min(r.max, (long)atoi(e))); break;
      case Env::zero_min: if (*e && v == 0) f = (int)r.min; break;
      case Env::count_min: if (*e && v >= 0) f = (int)(v == 0 ? r.min : top); break;
      case Env::count: if (*e && v > 0) f = (int)top; break;
      case Env::exact: if (*e && v >= r.min && v <= r.max) f = (int)v; break;
    }
  }
}

static const OptionRow* find(const char* key) {
  for (const OptionRow& r : kOptions)
    if (r.key && key && !std::strcmp(r.key, key)) return &r;
  fail(KP2D_ERR_ARG, "unknown option '%s'", key ? key : "(null)");
  return nullptr;
}

int set_option(Options& o, const char* key, long value) {
  const OptionRow* r = find(key);
  if (!r) return KP2D_ERR_ARG;
  if (value < r->min || value > r->max) return fail(KP2D_ERR_ARG, "%s is %ld .. %ld", r->key, r->min, r->max);
  o.*r->field = (r->field == &Options::lanes && value == 0) ? o.lanes_default : (int)value;
  return KP2D_OK;
}

int get_option(const Options& o, const char* key, long* value) {
  const OptionRow* r = find(key);
  if (!r) return KP2D_ERR_ARG;
  if (!value) return fail(KP2D_ERR_ARG, "null argument");
  *value = o.*r->field;
  return KP2D_OK;
}

const char* option_name(int index) {
  for (const OptionRow& r : kOptions)
    if (r.key && index >= 0 && index-- == 0) return r.key;
  return nullptr;
}

Tuning tuning_from_env(const char* (*get)(const char*)) {
  auto on = [get](const char* name) { const char* e = get(name); return !(e && e[0] == '0'); };
  auto num = [get](const char* name, long def) { const char* e = get(name); return e ? atol(e) : def; };
  Tuning t;
  t.match_mfma = on("KP2D_MATCH_MFMA");
  t.topk_small = (int)num("KP2D_TOPK_SMALL", TOPK_SMALL_MAX);
  t.gather_lds = on("KP2D_GATHER_LDS");
  t.vlad_px = (int)num("KP2D_VLAD_PX", 320);
  t.vlad_split = on("KP2D_VLAD_SPLIT");
  t.att_ksplit = num("KP2D_ATT_KSPLIT", 256);
  t.att_q = (int)num("KP2D_ATT_Q", 256);
  t.att_affine = on("KP2D_ATT_AFFINE");
  t.lg_fuse = on("KP2D_LG_FUSE");
  t.lg_fuse_next = on("KP2D_LG_FUSE_NEXT");
  t.lg_tail_nw = (int)num("KP2D_LG_TAIL_NW", 0);
  t.seg_ids_only = on("KP2D_SEG_IDS_ONLY");
  return t;
}

const Tuning& tuning() {
  static const Tuning t = tuning_from_env([](const char* name) -> const char* { return getenv(name); });
  return t;
}

}  // namespace kp2d

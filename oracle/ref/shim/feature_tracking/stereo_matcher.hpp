// Shadow of feature_tracking/stereo_matcher.hpp: the names only; the fields are those the PatchMatch test assigns.
// MatchRectified() is a compile-only stub (reached from Patchmatch::Initialize alone) and aborts if it ever runs.
#pragma once

#include <cstdlib>
#include <vector>

#include "core/macros.hpp"
#include "params/params_base.hpp"
#include "vision_core/cv_types.hpp"

namespace bm {
namespace ft {

using namespace core;

class StereoMatcher final {
 public:
  struct Params final : public ParamsBase {
    MACRO_PARAMS_STRUCT_CONSTRUCTORS(Params);
    int templ_cols = 31;
    int templ_rows = 11;
    int max_disp = 128;
    double max_matching_cost = 0.15;
    bool bidirectional = false;
    bool subpixel_refinement = false;

   private:
    void LoadParams(const YamlParser&) override { std::abort(); }
  };

  explicit StereoMatcher(const Params&) {}

  std::vector<double> MatchRectified(const Image1b&, const Image1b&, const VecPoint2f&) { std::abort(); }
};

}  // namespace ft
}  // namespace bm

// Shadow of feature_tracking/feature_detector.hpp: the names only.  Detect() is a compile-only stub: it is reached from
// Patchmatch::Initialize alone, which nothing here calls (the seeder is out of scope), and aborts if it ever runs.
#pragma once

#include <cstdlib>

#include "core/macros.hpp"
#include "params/params_base.hpp"
#include "vision_core/cv_types.hpp"

namespace bm {
namespace ft {

using namespace core;

class FeatureDetector final {
 public:
  struct Params final : public ParamsBase {
    MACRO_PARAMS_STRUCT_CONSTRUCTORS(Params);
    int max_features_per_frame = 200;

   private:
    void LoadParams(const YamlParser&) override { std::abort(); }
  };

  explicit FeatureDetector(const Params&) {}

  void Detect(const Image1b&, const VecPoint2f&, VecPoint2f&) { std::abort(); }
};

}  // namespace ft
}  // namespace bm

// Shadow of params/params_base.hpp: the names only.  Parameters are set field by field here, never parsed.
#pragma once

#include <cstdlib>
#include <string>

#include <opencv2/core.hpp>

#include "params/yaml_parser.hpp"

namespace bm {
namespace core {

class ParamsBase {
 public:
  ParamsBase() = default;
  virtual ~ParamsBase() = default;
  void Parse(const cv::FileNode&, const cv::FileNode& = cv::FileNode()) { std::abort(); }
  void Parse(const std::string&, const std::string& = "") { std::abort(); }
  void Parse(const YamlParser&) { std::abort(); }

 protected:
  virtual void LoadParams(const YamlParser& parser) = 0;
};

}  // namespace core
}  // namespace bm

// Shadow of params/yaml_parser.hpp (which needs yaml-cpp and Eigen): the names only.
#pragma once

#include <string>

namespace bm {
namespace core {

class YamlParser {
 public:
  YamlParser() = default;
  YamlParser Subtree(const std::string&) const { return YamlParser(); }
};

}  // namespace core
}  // namespace bm

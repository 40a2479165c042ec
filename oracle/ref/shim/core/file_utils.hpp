// Shadow: the reference header of this name needs Boost; the PatchMatch test uses nothing from it but the logging
// macros it brings along.
#pragma once

#include <glog/logging.h>

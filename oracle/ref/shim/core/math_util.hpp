// Shadow: the reference header of this name needs Eigen / Boost; the PatchMatch test uses nothing from it.
#pragma once

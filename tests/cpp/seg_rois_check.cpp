// Test helper: the ROI entries of the C++ class surface (InstanceFusion::ProcessSegmentationRois / ProcessSegmentationDeferredRois), built with plain g++ and no
// HIP header.  Without a GPU the map cannot be created and both calls must refuse loudly; with one, an empty call goes through and roi_size = 65 and n = 257 are
// refused with the library's messages.
//   seg_rois_check   -> "refused: <message>" "refused deferred: <message>"  or  "created" "refused 65: <message>" "refused 257: <message>"
#include <cstdio>

#include "ifx_host.hpp"

int main()
{
    Resolution::getInstance(64, 48);
    Intrinsics::getInstance(50.f, 50.f, 32.f, 24.f);
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 100000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(IFX_NUM_INSTANCES, 64, 48);
    try {
        inst.ProcessSegmentationRois(map, nullptr, 28, nullptr, 0.5f, nullptr, 0, 0, false, nullptr);
        std::printf("created\n");
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        try {
            inst.ProcessSegmentationDeferredRois(map, 0, nullptr, 28, nullptr, 0.5f, nullptr, 0, 0, false, nullptr);
            std::printf("accepted deferred\n");
        } catch (const std::exception& e2) {
            std::printf("refused deferred: %s\n", e2.what());
        }
        return 0;
    }
    try {
        inst.ProcessSegmentationRois(map, nullptr, 65, nullptr, 0.5f, nullptr, 0, 0, false, nullptr);
        std::printf("accepted 65\n");
    } catch (const std::exception& e) {
        std::printf("refused 65: %s\n", e.what());
    }
    try {
        inst.ProcessSegmentationRois(map, nullptr, 28, nullptr, 0.5f, nullptr, 257, 0, false, nullptr);
        std::printf("accepted 257\n");
    } catch (const std::exception& e) {
        std::printf("refused 257: %s\n", e.what());
    }
    return 0;
}

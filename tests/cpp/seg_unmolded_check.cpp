// Test helper: the default detector's entries of the C++ class surface (InstanceFusion::ProcessSegmentationUnmolded / ProcessSegmentationDeferredUnmolded,
// ElasticFusion::UnmoldDetections, InstanceFusion::MoldedInputSize / DetectorInputMolded), built with plain g++ and no HIP header.  The size rule runs
// anywhere.  Without a GPU the map cannot be created and the calls must refuse loudly; with one, an empty call goes through and M = 65, R = 257 and an empty
// window are refused with the library's messages.
//   seg_unmolded_check   -> "size <8 numbers>" then "refused: <message>" "refused deferred: <message>" "refused input: <message>"
//                           or "created 0" "refused 65: <message>" "refused 257: <message>" "refused window: <message>" "refused input: <message>"
#include <cstdio>

#include "ifx_host.hpp"

int main()
{
    int32_t o[8];
    InstanceFusion::MoldedInputSize(640, 480, 800, 1024, o);
    std::printf("size %d %d %d %d %d %d %d %d\n", o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
    try {
        InstanceFusion::MoldedInputSize(640, 480, 0, 19, o);
        std::printf("accepted size\n");
    } catch (const std::exception& e) {
        std::printf("refused size: %s\n", e.what());
    }
    Resolution::getInstance(64, 48);
    Intrinsics::getInstance(50.f, 50.f, 32.f, 24.f);
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 100000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(IFX_NUM_INSTANCES, 64, 48);
    const int32_t window[4] = {o[4], o[5], o[6], o[7]}, empty[4] = {5, 0, 5, 64};
    const double mean[3] = {123.7, 116.8, 103.9};
    int32_t kept = -1;
    try {
        const int k = inst.ProcessSegmentationUnmolded(map, nullptr, nullptr, window, nullptr, 0, 28, 81, IFX_UNMOLD_NHWC, 0, false, nullptr);
        std::printf("created %d\n", k);
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        try {
            inst.ProcessSegmentationDeferredUnmolded(map, 0, nullptr, nullptr, window, nullptr, 0, 28, 81, IFX_UNMOLD_NHWC, 0, false, nullptr);
            std::printf("accepted deferred\n");
        } catch (const std::exception& e2) {
            std::printf("refused deferred: %s\n", e2.what());
        }
        try {   // (no map, no ElasticFusion object: its UnmoldDetections is reached only with a GPU, below)
            inst.DetectorInputMolded(map, -1, 64, 64, mean, IFX_MOLD_NHWC, nullptr, 0, nullptr);
            std::printf("accepted input\n");
        } catch (const std::exception& e2) {
            std::printf("refused input: %s\n", e2.what());
        }
        return 0;
    }
    try {
        inst.ProcessSegmentationUnmolded(map, nullptr, nullptr, window, nullptr, 0, 65, 81, IFX_UNMOLD_NHWC, 0, false, nullptr);
        std::printf("accepted 65\n");
    } catch (const std::exception& e) {
        std::printf("refused 65: %s\n", e.what());
    }
    try {
        inst.ProcessSegmentationUnmolded(map, nullptr, nullptr, window, nullptr, 257, 28, 81, IFX_UNMOLD_NHWC, 0, false, nullptr);
        std::printf("accepted 257\n");
    } catch (const std::exception& e) {
        std::printf("refused 257: %s\n", e.what());
    }
    try {
        map->elasticFusion().UnmoldDetections(nullptr, nullptr, empty, nullptr, 0, 28, 81, IFX_UNMOLD_NCHW, 64, 48, nullptr, nullptr, nullptr, nullptr, nullptr, &kept, nullptr);
        std::printf("accepted window\n");
    } catch (const std::exception& e) {
        std::printf("refused window: %s\n", e.what());
    }
    try {
        inst.DetectorInputMolded(map, -1, 64, 64, nullptr, IFX_MOLD_NHWC, nullptr, 0, nullptr);
        std::printf("accepted input\n");
    } catch (const std::exception& e) {
        std::printf("refused input: %s\n", e.what());
    }
    return 0;
}

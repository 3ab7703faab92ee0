// Test helper: the device-mask entry of the C++ class surface (InstanceFusion::ProcessSegmentationDevice), built with plain g++ and no HIP header.
// Without a GPU the map cannot be created and the call must refuse loudly; with one, an empty call goes through and n = 257 is refused with the library's message.
//   seg_device_check   -> "refused: <message>"  or  "created" then "refused 257: <message>"
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
        inst.ProcessSegmentationDevice(map, nullptr, IFX_MASK_U8, 0.5f, nullptr, 0, 0, false, nullptr);
        std::printf("created\n");
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    try {
        inst.ProcessSegmentationDevice(map, nullptr, IFX_MASK_F32, 0.5f, nullptr, 257, 0, false, nullptr);
        std::printf("accepted 257\n");
    } catch (const std::exception& e) {
        std::printf("refused 257: %s\n", e.what());
    }
    return 0;
}

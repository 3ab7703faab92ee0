// Test helper: the headless map renders of the C++ host on a spatially sharded map (ElasticFusionInterface::RenderMapToBuffer / RenderMapIDToBuffer, which take
// ifx_owner_render_view when the host is sharded), built with plain g++ and no HIP header.
//   sharded_view_check   -> where there is no GPU: "refused: <message>" (Init fails, and RenderMapToBuffer throws instead of touching the buffers);
//                           otherwise "created", then the render of the empty map at a world of one (n_ranks = -1, the library's communicator):
//                           "empty <pixels with id -1 and the clear colour, alpha 0> of <pixels>" and "collectives <n> bytes <b>" (ifx_owner_exchange_stats)
#include <cstdio>

#include "ifx_host.hpp"

int main()
{
    const int w = 37, h = 29;
    Resolution::getInstance(64, 48);
    Intrinsics::getInstance(50.f, 50.f, 32.f, 24.f);
    ElasticFusionInterface map;
    Sharding shard;
    shard.ranks = -1;
    const bool ok = map.Init({}, 4096, 0, "./sharded_view_check", false, 10.f, shard);
    const Matrix4f pose = Matrix4f::Identity();
    const Matrix4f mvp = viewerMvp(40.0, 40.0, w / 2.0, h / 2.0, w, h, 0.1, 1000.0, pose);
    std::vector<float> rgba((size_t)w * h * 4, 7.f);
    std::vector<int32_t> ids((size_t)w * h, 7);
    if (!ok) {
        try {
            map.RenderMapToBuffer(mvp, w, h, true, false, false, rgba.data(), ids.data());
        } catch (const std::exception& e) {
            for (float v : rgba) if (v != 7.f) return 1;
            for (int32_t v : ids) if (v != 7) return 1;
            std::printf("refused: %s\n", e.what());
            return 0;
        }
        std::printf("RenderMapToBuffer did not refuse\n");
        return 1;
    }
    std::printf("created\n");
    int64_t st[2] = {0, 0};
    ifx_owner_exchange_stats(map.handle(), st, 1);
    map.RenderMapToBuffer(mvp, w, h, true, false, false, rgba.data(), ids.data());
    int empty = 0;
    for (int k = 0; k < w * h; k++) empty += ids[k] == -1 && rgba[k * 4] == 1.f && rgba[k * 4 + 1] == 1.f && rgba[k * 4 + 2] == 1.f && rgba[k * 4 + 3] == 0.f;
    ifx_owner_exchange_stats(map.handle(), st, 1);
    std::printf("empty %d of %d\ncollectives %lld bytes %lld\n", empty, w * h, (long long)st[0], (long long)st[1]);
    map.RenderMapIDToBuffer(mvp, w, h, ids.data());
    ifx_owner_exchange_stats(map.handle(), st, 1);
    std::printf("ids only: collectives %lld bytes %lld\n", (long long)st[0], (long long)st[1]);
    return 0;
}

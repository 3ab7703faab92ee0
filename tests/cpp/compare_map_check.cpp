// Test helper: the compare map's rule from the C++ class surface -- InstanceFusion::setCompareMapType / getCompareMapType / segmentationMatches / maskCompareMap --
// built with plain g++ and no HIP header.  On a GPU it repeats tests/test_gpu_compare_map.py's X scene: a sheet of one stable surfel per pixel (100 x 52), sixteen
// registered instance slots, instances 2 and 3 (one class) present on the two diagonals of one square, masks A = "\" and B = "/".
//   compare_map_check TYPE   ->  "refused: <message>"   (no GPU)
//                            or  "type T" / "best a b" / "target a b" / "stage a b"
#include <cstdio>
#include <cstdlib>

#include "ifx_host.hpp"

namespace {
const int W = 100, H = 52, NI = IFX_NUM_INSTANCES;

struct Fixed : MaskSource {
    MaskResult r;
    bool detect(int, const ImagePtr, int, int, MaskResult* out) override { *out = r; return true; }
};

void check(int r, ifx_t* h, const char* what)
{
    if (r < 0) throw std::runtime_error(std::string(what) + ": " + ifx_last_error(h));
}

struct Sheet {
    ifx_t* h;
    std::vector<unsigned char> rgb;
    std::vector<unsigned short> depth;
    float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    explicit Sheet(ifx_t* h_) : h(h_), rgb((size_t)W * H * 3), depth((size_t)W * H, 1500)
    {
        for (size_t k = 0; k < rgb.size(); k++) rgb[k] = (unsigned char)(30 + (k * 2654435761u >> 24) % 200);
    }
    void frame() { check(ifx_process_frame(h, rgb.data(), depth.data(), 0, eye, 1.f, nullptr), h, "ifx_process_frame"); }
    // download, edit(pc, votes, n), upload, the pose again, one frame: the id image shows the edited map
    template <typename F>
    void settle(F&& edit)
    {
        const int n = ifx_map_count(h);
        std::vector<float> pc((size_t)n * 4), nr((size_t)n * 4), col((size_t)n * 2), tm((size_t)n * 2), ic((size_t)n * 4), votes((size_t)n * 48);
        check(ifx_map_download(h, n, pc.data(), nr.data(), col.data(), tm.data(), ic.data(), votes.data()), h, "ifx_map_download");
        edit(pc, votes, n);
        check(ifx_map_upload(h, n, pc.data(), nr.data(), col.data(), tm.data(), ic.data(), votes.data()), h, "ifx_map_upload");
        check(ifx_set_pose(h, eye, ifx_tick(h)), h, "ifx_set_pose");
        frame();
    }
};
}   // namespace

int main(int argc, char** argv)
{
    const int type = argc > 1 ? std::atoi(argv[1]) : 2;
    Resolution::getInstance(W, H);
    Intrinsics::getInstance(80.f, 80.f, 50.f, 26.f);
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 100000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(NI, W, H);
    inst.setSuperpixelRefinement(false);
    try {
        inst.bindMap(map);
        inst.setCompareMapType(type);
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    try {
        ifx_t* h = map->handle();
        Sheet s(h);
        for (int i = 0; i < 3; i++) s.frame();
        s.settle([](std::vector<float>& pc, std::vector<float>& votes, int n) {
            for (int k = 0; k < n; k++) pc[(size_t)k * 4 + 3] = 20.f;
            std::fill(votes.begin(), votes.end(), 0.f);
        });
        auto src = std::make_shared<Fixed>();
        inst.setMaskSource(src);
        for (int c = 0; c < 16; c += 8) {   // slots c .. c + 7: eight 20 x 20 rectangles, classes 10 + slot / 2
            src->r.n = 8;
            src->r.masks.assign((size_t)8 * W * H, 0);
            src->r.class_ids.resize(8);
            for (int k = 0; k < 8; k++) {
                const int x0 = 3 + (k % 4) * 24, y0 = 3 + (k / 4) * 24;
                for (int y = y0; y < y0 + 20; y++) for (int x = x0; x < x0 + 20; x++) src->r.masks[((size_t)k * H + y) * W + x] = 255;
                src->r.class_ids[k] = 10 + (c + k) / 2;
            }
            inst.ProcessSegmentation(nullptr, nullptr, map, 10 + c, false);
        }
        std::vector<int32_t> ids((size_t)W * H);
        check(ifx_image_download(h, "ids_after", ids.data(), (int64_t)ids.size() * 4), h, "ifx_image_download");
        auto on_a = [](int x, int y) { return x >= 10 && x < 40 && y >= 10 && y < 40 && std::abs((y - 10) - (x - 10)) <= 1; };
        auto on_b = [](int x, int y) { return x >= 10 && x < 40 && y >= 10 && y < 40 && std::abs((y - 10) + (x - 10) - 29) <= 1; };
        s.settle([&](std::vector<float>&, std::vector<float>& votes, int n) {
            std::fill(votes.begin(), votes.end(), 0.f);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const int id = ids[(size_t)y * W + x];
                    if (id <= 0 || id >= n) continue;
                    votes[(size_t)id * 48 + 1] = (float)((on_a(x, y) ? 3 << 16 : 0) + (on_b(x, y) ? 3 : 0));   // word 1: instance 2 in the high half, 3 in the low one
                }
        });
        src->r.n = 2;
        src->r.masks.assign((size_t)2 * W * H, 0);
        src->r.class_ids = {11, 11};
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                if (on_a(x, y)) src->r.masks[(size_t)y * W + x] = 255;
                if (on_b(x, y)) src->r.masks[((size_t)H + y) * W + x] = 255;
            }
        int stage[2] = {-9, -9};
        inst.maskCompareMap(map, src->r.masks.data(), src->r.class_ids.data(), 2, nullptr, nullptr, nullptr, stage);
        inst.ProcessSegmentation(nullptr, nullptr, map, 200, false);
        const auto m = inst.segmentationMatches();
        std::printf("type %d\n", inst.getCompareMapType());
        std::printf("best"); for (int v : m.first) std::printf(" %d", v); std::printf("\n");
        std::printf("target"); for (int v : m.second) std::printf(" %d", v); std::printf("\n");
        std::printf("stage %d %d\n", stage[0], stage[1]);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    return 0;
}

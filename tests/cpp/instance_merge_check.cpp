// Test helper: InstanceFusion::checkLoopClosure / mergeInstances / findDuplicateInstances / resolveMergePairs from the C++ class surface, built with plain g++ and no
// HIP header.  On a GPU: a sheet of one stable surfel per pixel (100 x 52), eight registered instance slots, counters written surfel by surfel; the loop-closure
// table gets a chain (5 -> 3 -> 1) and 6 -> 0, checkLoopClosure merges, and the map before and after goes to OUT for the Python side to repeat.
//   instance_merge_check OUT   ->  "refused: <message>"   (no GPU)
//                              or  "n N" / "resolved 3>1 5>1 6>0" / "column4 reset" / "duplicates ..."; OUT: int32 n, then float32 votes[n*48] col[n*2] tm[n*2] as
//                                  uploaded, votes[n*48] col[n*2] afterwards, int32 table[96] afterwards
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

struct Map {
    int n = 0;
    std::vector<float> pc, nr, col, tm, ic, votes;
    void get(ifx_t* h)
    {
        n = ifx_map_count(h);
        pc.resize((size_t)n * 4); nr.resize((size_t)n * 4); col.resize((size_t)n * 2); tm.resize((size_t)n * 2); ic.resize((size_t)n * 4); votes.resize((size_t)n * 48);
        check(ifx_map_download(h, n, pc.data(), nr.data(), col.data(), tm.data(), ic.data(), votes.data()), h, "ifx_map_download");
    }
    void put(ifx_t* h) { check(ifx_map_upload(h, n, pc.data(), nr.data(), col.data(), tm.data(), ic.data(), votes.data()), h, "ifx_map_upload"); }
};
}   // namespace

int main(int argc, char** argv)
{
    const char* out_path = argc > 1 ? argv[1] : "instance_merge_check.bin";
    {   // host only: chains resolve to their roots, a cycle throws
        const auto r = InstanceFusion::resolveMergePairs({{5, 3}, {3, 1}, {6, 0}});
        if (r != std::vector<std::pair<int, int>>{{3, 1}, {5, 1}, {6, 0}}) { std::printf("failed: resolveMergePairs\n"); return 1; }
        bool threw = false;
        try { InstanceFusion::resolveMergePairs({{1, 2}, {2, 1}}); } catch (const std::exception&) { threw = true; }
        if (!threw) { std::printf("failed: a cycle was accepted\n"); return 1; }
    }
    Resolution::getInstance(W, H);
    Intrinsics::getInstance(80.f, 80.f, 50.f, 26.f);
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 100000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(NI, W, H);
    inst.setSuperpixelRefinement(false);
    try {
        inst.bindMap(map);
        inst.mergeInstances({});
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    try {
        ifx_t* h = map->handle();
        std::vector<unsigned char> rgb((size_t)W * H * 3);
        std::vector<unsigned short> depth((size_t)W * H, 1500);
        for (size_t k = 0; k < rgb.size(); k++) rgb[k] = (unsigned char)(30 + (k * 2654435761u >> 24) % 200);
        float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        auto frame = [&]() { check(ifx_process_frame(h, rgb.data(), depth.data(), 0, eye, 1.f, nullptr), h, "ifx_process_frame"); };
        for (int i = 0; i < 3; i++) frame();
        Map m;
        m.get(h);
        for (int k = 0; k < m.n; k++) m.pc[(size_t)k * 4 + 3] = 20.f;
        std::fill(m.votes.begin(), m.votes.end(), 0.f);
        m.put(h);
        check(ifx_set_pose(h, eye, ifx_tick(h)), h, "ifx_set_pose");
        frame();
        auto src = std::make_shared<Fixed>();
        inst.setMaskSource(src);
        src->r.n = 8;   // slots 0 .. 7: eight 20 x 20 rectangles, classes 10 + slot / 2
        src->r.masks.assign((size_t)8 * W * H, 0);
        src->r.class_ids.resize(8);
        for (int k = 0; k < 8; k++) {
            const int x0 = 3 + (k % 4) * 24, y0 = 3 + (k / 4) * 24;
            for (int y = y0; y < y0 + 20; y++) for (int x = x0; x < x0 + 20; x++) src->r.masks[((size_t)k * H + y) * W + x] = 255;
            src->r.class_ids[k] = 10 + k / 2;
        }
        inst.ProcessSegmentation(nullptr, nullptr, map, 10, false);
        std::vector<int> table((size_t)NI * 5);
        inst.getLoopClosureInstanceTable(table.data());
        m.get(h);
        for (int k = 0; k < m.n; k++) {   // counters of instances 0 .. 7 (words 0 .. 3), every seventh surfel a first-frame one; colours: the table's, the default, none
            for (int w = 0; w < 4; w++) m.votes[(size_t)k * 48 + w] = k % 7 == 3 ? -1.f : (float)((((k * 7 + w) % 50) << 16) + (k * 3 + w) % 40);
            const int c = k % 10;
            m.col[(size_t)k * 2 + 1] = c < 8 ? (float)((table[(size_t)c * 5] << 16) + (table[(size_t)c * 5 + 1] << 8) + table[(size_t)c * 5 + 2]) : c == 8 ? 7434609.f : 0.f;
        }
        m.put(h);
        Map before;
        before.get(h);
        table[5 * 5 + 4] = 3; table[3 * 5 + 4] = 1; table[6 * 5 + 4] = 0;
        inst.checkLoopClosure(table.data(), map);
        bool reset = true;
        for (int i = 0; i < NI; i++) reset = reset && table[(size_t)i * 5 + 4] == i;
        Map after;
        after.get(h);
        std::vector<int32_t> cls(NI);
        check(ifx_instance_table(h, cls.data()), h, "ifx_instance_table");
        FILE* f = std::fopen(out_path, "wb");
        if (!f) throw std::runtime_error(std::string("cannot write ") + out_path);
        const int32_t n = before.n;
        std::fwrite(&n, 4, 1, f);
        std::fwrite(before.votes.data(), 4, before.votes.size(), f); std::fwrite(before.col.data(), 4, before.col.size(), f); std::fwrite(before.tm.data(), 4, before.tm.size(), f);
        std::fwrite(after.votes.data(), 4, after.votes.size(), f); std::fwrite(after.col.data(), 4, after.col.size(), f);
        std::fwrite(cls.data(), 4, cls.size(), f);
        std::fclose(f);
        std::printf("n %d %d\n", before.n, after.n);
        std::printf("column4 %s\n", reset ? "reset" : "kept");
        check(ifx_set_pose(h, eye, ifx_tick(h)), h, "ifx_set_pose");
        frame();
        std::printf("duplicates");
        for (const auto& p : inst.findDuplicateInstances(map)) std::printf(" %d>%d", p.first, p.second);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    return 0;
}

// vtk_shim.cpp -- l3k::ExportDefinition / l3k::PvtuExporter (include/l3k/operator.hpp) used the way the reference's examples end:
// an exporter on the mesh, an export definition with named field groups, exportSolution.  The mesh is 3 x 2 x 2 hexes of order 2
// with perturb = 0.1; the field storage (4 rows, ld = local nodes + 5) is read from argv[1] (raw doubles, written by the Python test
// so that both routes export the same bits) and the files go to argv[2] with a chunk of 4096 text bytes.  tests/test_cpp_vtk.py
// compares them byte for byte with the Python route's.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/vtk_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/vtk_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    constexpr int   p = 2, n_fields = 4;
    l3k::Context    ctx{0};
    l3k::CubeMesh   mesh{{3, 2, 2}, p, {1, 1, 1}, 0, 0.1};
    l3k::DeviceMesh dmesh{ctx, mesh, 1};
    const size_t    ld       = size_t(mesh.nLocalNodes()) + 5;
    int             failures = 0;

    std::vector< double > fields(ld * n_fields);
    for (size_t i = 0; i < fields.size(); ++i)
        fields[i] = double(i % 97) / 7.;
    if (argc > 1)
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(fields.data(), sizeof(double), fields.size(), f) != fields.size())
            ++failures;
        if (f)
            std::fclose(f);
    }
    double* d_fields = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d_fields), fields.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(d_fields, fields.data(), fields.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }

    l3k::PvtuExporter exporter{dmesh, 0, 1, 4096};
    const auto        info = exporter.info();
    failures += info.n_points != mesh.nLocalNodes() || info.n_cells != 12 * p * p * p || info.n_conn != 8 * info.n_cells || info.chunk_bytes != 4096;

    l3k::ExportDefinition export_def{argc > 2 ? argv[2] : "vtk_shim_out/solution.pvtu"};
    export_def.defineField("T", {2});
    export_def.defineField("flux", {3, 0});
    const std::vector< int > velocity{1, 3, 0};
    export_def.defineField("velocity", velocity);
    failures += export_def.size() != 3;
    exporter.exportSolution(export_def, d_fields, ld, n_fields);

    // a refused export throws with the reference's message
    l3k::ExportDefinition four{"vtk_shim_out/never.pvtu"};
    four.defineField("w", {0, 1, 2, 3});
    bool threw = false;
    try
    {
        exporter.exportSolution(four, d_fields, ld, n_fields);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("Field groupings must have size") != std::string::npos;
    }
    failures += !threw;
    l3k::PvtuExporter moved{std::move(exporter)};
    failures += moved.info().n_points != info.n_points;

    (void)hipFree(d_fields);
    std::printf("l3k::PvtuExporter: %lld points, %lld cells, chunk %zu\n", (long long)info.n_points, (long long)info.n_cells, info.chunk_bytes);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}

// vtk_text_driver.cpp -- sanitizer driver for the host side of the ParaView export (l3ster_amd/csrc/host/vtk_text.cpp): sizes, the
// 2^32 guard, the argument checks, the file names and both XML texts through the C entry points, with the size query, buffers of
// exactly the needed length and buffers that are too small.  Built with -fsanitize=address,undefined by tests/test_vtk_cpu.py;
// the error text goes through the setError of this file, since the library's lives in a translation unit that needs HIP.
#include "host/vtk_text.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace l3k::dev
{
static char last_error[1024];
void        setError(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
} // namespace l3k::dev

int main()
{
    int bad = 0;
    // sizes of every shape the library runs, and the guard on both counts
    for (int dim = 2; dim <= 3; ++dim)
        for (int p = 1; p <= 8; ++p)
        {
            l3k_vtk_info i{};
            bad += l3k_vtk_sizes(dim, p, 7, 1000, &i) != 0;
            int64_t per = 1;
            for (int d = 0; d < dim; ++d)
                per *= p;
            bad += i.n_cells != 7 * per || i.n_conn != i.n_cells * (dim == 2 ? 4 : 8) || i.encoded_bytes[3] != 4 * ((8 + uint64_t(i.n_cells) + 2) / 3);
            const int64_t most = int64_t(0xffffffffull / uint64_t(per * (dim == 2 ? 4 : 8)));
            bad += l3k_vtk_sizes(dim, p, most, 0xffffffffll, &i) != 0;
            bad += l3k_vtk_sizes(dim, p, most + 1, 1, &i) != -1 || !std::strstr(l3k::dev::last_error, "connectivity entries");
            bad += l3k_vtk_sizes(dim, p, 1, 0x100000000ll, &i) != -1 || !std::strstr(l3k::dev::last_error, "4294967296 local nodes");
            bad += l3k_vtk_sizes(dim, p, INT64_MAX, 1, &i) != -1;
        }
    bad += l3k_vtk_sizes(3, 2, 1, 1, nullptr) != -1;

    // the texts: size query, exact buffer, short buffer
    const char*    names[] = {"T", "a rather long name for a flux vector", "w"};
    const int      rows[]  = {1, 2, 3};
    const uint64_t enc[4]  = {44, 100, 24, 16};
    for (int n_groups = 0; n_groups <= 3; ++n_groups)
        for (const char* path : {"out.pvtu", "some/dir/out", "a.b/c.d.e", ""})
        {
            size_t need = 0;
            bad += l3k_vtk_pvtu_text(path, 3, n_groups, names, rows, nullptr, 0, &need) != 0 || need == 0;
            std::vector< char > buf(need);
            bad += l3k_vtk_pvtu_text(path, 3, n_groups, names, rows, buf.data(), buf.size(), nullptr) != 0;
            bad += std::string(buf.begin(), buf.end()).find("</VTKFile>") == std::string::npos;
            if (need > 1)
                bad += l3k_vtk_pvtu_text(path, 3, n_groups, names, rows, buf.data(), need - 1, &need) != -1;
            bad += l3k_vtk_vtu_header_text(9, 4, enc, n_groups, names, rows, nullptr, 0, &need) != 0;
            std::vector< char > head(need);
            bad += l3k_vtk_vtu_header_text(9, 4, enc, n_groups, names, rows, head.data(), head.size(), &need) != 0 || head.back() != '_';
            (void)l3k::host::vtkVtuFileName(path, 2);
            (void)l3k::host::vtkPvtuFileName(path);
        }
    // the refusals
    const int         inds[] = {0, 1, 2, 3, 4, 5};
    const int         zero_rows[] = {1, 0, 3}, four_rows[] = {1, 4, 1};
    const char*       evil[] = {"T", "a<b", "w"};
    const char*       empty[] = {"T", "", "w"};
    const std::string ok     = l3k::host::vtkCheckGroups(0, 1, 3, names, rows, inds, 6);
    bad += !ok.empty();
    bad += l3k::host::vtkCheckGroups(0, 1, 3, names, zero_rows, inds, 6).find("Field groupings") != 0;
    bad += l3k::host::vtkCheckGroups(0, 1, 3, names, four_rows, inds, 6).find("Field groupings") != 0;
    bad += l3k::host::vtkCheckGroups(0, 1, 3, names, rows, inds, 5) != "Out of bounds index";
    bad += l3k::host::vtkCheckGroups(1, 1, 3, names, rows, inds, 6).find("rank 1") != 0;
    bad += l3k::host::vtkCheckGroups(-1, 2, 3, names, rows, inds, 6).find("rank -1") != 0;
    bad += l3k::host::vtkCheckGroups(0, 1, 3, evil, rows, inds, 6).find("name of field group 1") != 0;
    bad += l3k::host::vtkCheckGroups(0, 1, 3, empty, rows, inds, 6).find("name of field group 1") != 0;
    bad += l3k::host::vtkCheckGroups(0, 1, 3, nullptr, rows, inds, 6).empty();
    bad += l3k_vtk_pvtu_text("x", 2, 3, evil, rows, nullptr, 0, nullptr) != -1;
    size_t need = 0;
    bad += l3k_vtk_pvtu_text("x", 2, 3, evil, rows, nullptr, 0, &need) != -1;
    bad += l3k_vtk_pvtu_text(nullptr, 2, 3, names, rows, nullptr, 0, &need) != -1;
    bad += l3k_vtk_vtu_header_text(9, 4, nullptr, 0, names, rows, nullptr, 0, &need) != -1;
    if (bad)
    {
        std::printf("vtk text driver: %d violations (%s)\n", bad, l3k::dev::last_error);
        return 1;
    }
    std::printf("vtk text driver: ok\n");
    return 0;
}

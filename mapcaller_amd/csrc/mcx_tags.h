// mapcaller_amd/csrc/mcx_tags.h — the argument of -rg (include/mcx.h at mcx_rg_parse): bwa mem -R's form taken apart and checked.  Plain C++, no HIP: the command
// line, the file front end and tests/hostemu/tags_check.cpp compile the same text.
//   every two-character sequence "\t" becomes a TAB; the line begins with "@RG" TAB; every further TAB-separated field is [A-Za-z][A-Za-z0-9] ':' and at least one
//   byte; exactly one field is ID; no byte below 0x20 but TAB, none 0x7f; the ID at most 255 bytes, the line at most 4096.
#ifndef MCX_TAGS_H
#define MCX_TAGS_H
#include <string>

namespace mcx {

enum { kRgMaxId = 255, kRgMaxLine = 4096 };

// arg -> line (real TABs, no newline) and its ID; false with the reason in words
static inline bool rg_parse(const char *arg, std::string &line, std::string &id, std::string &why)
{
    line.clear(); id.clear(); why.clear();
    if (!arg) { why = "no read-group line"; return false; }
    for (const char *p = arg; *p; p++) {
        if (p[0] == '\\' && p[1] == 't') { line += '\t'; p++; }
        else line += *p;
    }
    if (line.size() > (size_t)kRgMaxLine) { why = "the read-group line is longer than 4096 bytes"; return false; }
    for (unsigned char ch : line)
        if ((ch < 0x20 && ch != '\t') || ch == 0x7f) { why = "the read-group line holds a control byte (only TAB, or \\t, separates its fields)"; return false; }
    if (line.compare(0, 4, "@RG\t") != 0) { why = "the read-group line must begin with @RG and a TAB (-rg '@RG\\tID:x\\tSM:y')"; return false; }
    auto letter = [](unsigned char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
    auto digit = [](unsigned char ch) { return ch >= '0' && ch <= '9'; };
    int ids = 0;
    for (size_t at = 4; at <= line.size();) {
        size_t end = line.find('\t', at);
        if (end == std::string::npos) end = line.size();
        const size_t n = end - at;
        if (n < 4 || !letter((unsigned char)line[at]) || !(letter((unsigned char)line[at + 1]) || digit((unsigned char)line[at + 1])) || line[at + 2] != ':') {
            why = "a field of the read-group line is not KEY:value (two characters, a colon, at least one byte): '" + line.substr(at, n) + "'";
            return false;
        }
        if (line[at] == 'I' && line[at + 1] == 'D') { ids++; id = line.substr(at + 3, n - 3); }
        at = end + 1;
    }
    if (ids != 1) { why = ids ? "the read-group line has more than one ID field" : "the read-group line has no ID field"; id.clear(); return false; }
    if (id.size() > (size_t)kRgMaxId) { why = "the read group's ID is longer than 255 bytes"; id.clear(); return false; }
    return true;
}

} // namespace mcx
#endif

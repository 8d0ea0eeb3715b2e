/* dash_text.h -- the one-file reader shared by dash_read_dirs_text (dash_text.c) and the
   reader threads of dash_load_dirs_device (dash_load.cpp). Internal: not part of dash.h. */
#ifndef DASH_TEXT_H
#define DASH_TEXT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Only the first 19 * max_instr bytes of a core_<n>.txt can matter (dash_parse_core_text). */
static inline uint64_t dash_text_limit(uint32_t max_instr) { return 19ull * max_instr; }

/* Reads at most `limit` bytes of `path`. dst == NULL: measures (*got = what a read would
   return). Otherwise reads into dst[0..room); a file whose share does not fit gives
   DASH_EINVAL with *got = the room it needs. A file that cannot be opened gives DASH_EIO after
   the stderr line dash_parse_core_file prints (ref :827). */
int dashi_read_text_file(const char *path, uint64_t limit, char *dst, uint64_t room, uint64_t *got);

#ifdef __cplusplus
}
#endif
#endif

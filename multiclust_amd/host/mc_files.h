/*
 * mc_files.h -- the file plumbing of the host side, one copy of each part (mc_cli.h, which includes this file behind the types it
 * needs, says what each function does): the path of a result file, opening and closing one, a whole file into memory, the white
 * space and tokens of the text formats, the lines of a text that hold anything, the clock behind MC_READER_TIMING, and the two
 * writers every filter of a fileset ends in -- the kept lines of a .bim / .fam file and the lists of the entries kept and removed.
 * libc only, and static inline: a unit that is built as a program of its own (the drivers under tests/ compile mc_ld.c, mc_king.c,
 * mc_resid.c, ... each alone) has what it uses without naming another source file, and what it does not use is not emitted.
 * tests/files_host_driver.c runs these functions as a program of their own.  The messages carry the origin the caller passes, the
 * name of its source file, in front of the function's name here: a reader of stderr sees who wanted the file.
 */
#ifndef MC_FILES_H
#define MC_FILES_H

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static inline int mc_is_blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }
typedef struct mc_lines { char *line, *first, *end, *stop, *eof; } mc_lines;
typedef void (*mc_list_entry_fn)(FILE *fp, const void *arg, int v);

__attribute__((format(printf, 4, 5)))
static inline size_t mc_result_path(const mc_cli_options *opt, char *out, size_t n, const char *suffix, ...)
{
	if (opt->outfile_name) {
		snprintf(out, n, "%s", opt->outfile_name);
	} else {
		const size_t pl = strlen(opt->path);
		const int sep = pl && opt->path[pl - 1] != '/' && opt->path[pl - 1] != '\\';
		snprintf(out, n, "%s%s%s", opt->path, sep ? "/" : "", opt->filename_file);
	}
	const size_t len = strlen(out);		/* (of what fitted: a stem longer than the buffer is cut, and so is every suffix behind it) */
	va_list ap;
	va_start(ap, suffix);
	vsnprintf(out + len, n - len, suffix, ap);
	va_end(ap);
	return len;
}

static inline FILE *mc_open_result(const char *origin, const char *path, const char *mode)
{
	FILE *fp = fopen(path, mode);
	if (!fp) fprintf(stderr, "ERROR [%s::open_out]: could not open file '%s'\n", origin, path);
	return fp;
}

static inline int mc_close_result(FILE *fp)
{
	int bad = ferror(fp);
	if (fclose(fp)) bad = 1;
	return bad ? MC_EXIT_FILE_OPEN_ERROR : 0;
}

static inline char *mc_path_of(const char *prefix, const char *ext)
{
	char *p = malloc(strlen(prefix) + strlen(ext) + 1);
	if (p) { strcpy(p, prefix); strcat(p, ext); }
	return p;
}

static inline int mc_slurp(const char *origin, const char *path, char **out, size_t *size)
{
	FILE *f = fopen(path, "rb");
	const char *why = "could not open file '%s'";
	int rc = MC_EXIT_FILE_OPEN_ERROR;
	char *buf = NULL;
	*out = NULL;
	if (f) {
		fseek(f, 0, SEEK_END);
		const long n = ftell(f);
		fseek(f, 0, SEEK_SET);
		why = "out of memory reading '%s'";
		rc = MC_EXIT_MEMORY_ALLOCATION;
		if (n >= 0 && (buf = malloc((size_t)n + 1))) {
			why = "short read on '%s'";
			rc = fread(buf, 1, (size_t)n, f) == (size_t)n ? 0 : MC_EXIT_FILE_FORMAT_ERROR;
			buf[n] = 0;
			*size = (size_t)n;
		}
		fclose(f);
	}
	if (rc) {
		free(buf);
		fprintf(stderr, "ERROR [%s::slurp]: ", origin);
		fprintf(stderr, why, path);
		fprintf(stderr, "\n");
		return rc;
	}
	*out = buf;
	return 0;
}

static inline char *mc_dup_token(const char *s, size_t len)
{
	char *r = malloc(len + 1);
	if (r) { memcpy(r, s, len); r[len] = 0; }
	return r;
}

static inline double mc_now_s(void)
{
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static inline double mc_timing_line(const char *origin, const char *what, double t_start)
{
	const double t = mc_now_s();
	if (getenv("MC_READER_TIMING")) fprintf(stderr, "INFO [%s]: %-18s %.3f s\n", origin, what, t - t_start);
	return t;
}

static inline void mc_lines_start(mc_lines *it, char *text, size_t n)
{
	memset(it, 0, sizeof *it);
	it->stop = text;
	it->eof = text + n;
}

static inline int mc_lines_next(mc_lines *it)
{
	for (char *p = it->stop; p < it->eof; p = it->stop) {
		char *q = memchr(p, '\n', (size_t)(it->eof - p)), *s = p;
		if (!q) q = it->eof;
		it->stop = q < it->eof ? q + 1 : q;
		while (s < q && mc_is_blank(*s)) s++;
		if (s == q) continue;
		it->line = p;
		it->first = s;
		it->end = q;
		return 1;
	}
	return 0;
}

static inline int mc_copy_kept_lines(const char *origin, const char *from, const char *to, const int *kept, int n)
{
	char *buf;
	size_t size;
	int rc = mc_slurp(origin, from, &buf, &size);
	if (rc) return rc;
	FILE *fp = mc_open_result(origin, to, "wb");
	if (!fp) { free(buf); return MC_EXIT_FILE_OPEN_ERROR; }
	mc_lines it;
	mc_lines_start(&it, buf, size);
	for (int v = 0, x = 0; x < n && mc_lines_next(&it); v++)
		if (kept[x] == v) { x++; fwrite(it.line, 1, (size_t)(it.stop - it.line), fp); }
	rc = mc_close_result(fp);
	free(buf);
	return rc;
}

static inline int mc_write_kept_lists(const mc_cli_options *opt, const char *origin, const char *suffix, int n_file, int n_kept, const int *kept,
			mc_list_entry_fn print, const void *arg)
{
	char path[4400];
	FILE *in, *out;
	mc_result_path(opt, path, sizeof path, "%s.in", suffix);
	if (!(in = mc_open_result(origin, path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	mc_result_path(opt, path, sizeof path, "%s.out", suffix);
	if (!(out = mc_open_result(origin, path, "w"))) { fclose(in); return MC_EXIT_FILE_OPEN_ERROR; }
	for (int v = 0, x = 0; v < n_file; v++) {
		const int is_kept = x < n_kept && kept[x] == v;
		print(is_kept ? in : out, arg, v);
		x += is_kept;
	}
	const int rc_in = mc_close_result(in), rc_out = mc_close_result(out);
	return rc_in ? rc_in : rc_out;
}

#endif

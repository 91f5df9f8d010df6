/*
 * files_host_driver.c -- TEST INFRASTRUCTURE: mc_files.h as a program of its own, built plain and with -fsanitize=address,undefined by
 * tests/test_files_cpu.py.  Every buffer is allocated at exactly the size the test names, so a byte written behind one is an error
 * of the sanitized build.
 *
 *   files_host_driver path <n> <o> <d> <file>      the result path in a buffer of n bytes; o = "-": no -o.  Prints the length of the
 *                                                  stem, the path, and the path after each of two rewrites of the suffix
 *   files_host_driver open <origin> <path>         mc_open_result for writing; prints "open" or "NULL" (the line on stderr is the test's)
 *   files_host_driver slurp <origin> <path>        prints the status of mc_slurp, and the size read
 *   files_host_driver lines <file>                 prints the number of lines that hold anything but white space, then per line the
 *                                                  offsets of line, first, end and stop
 *   files_host_driver copy <from> <to> [v ...]     mc_copy_kept_lines with the map v ...; prints its status
 *   files_host_driver lists <stem> <n_file> [v ...]  mc_write_kept_lists on <stem>.kept.in / .out, entry v written as "e<v>"; prints
 *                                                  its status
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

static void print_entry(FILE *fp, const void *arg, int v) { fprintf(fp, "%s%d\n", (const char *)arg, v); }

static int *map_of(int n, char **argv)
{
	int *map = malloc(sizeof(int) * (size_t)(n ? n : 1));
	for (int x = 0; map && x < n; x++) map[x] = atoi(argv[x]);
	return map;
}

int main(int argc, char **argv)
{
	mc_cli_options opt;
	memset(&opt, 0, sizeof opt);
	if (argc == 6 && !strcmp(argv[1], "path")) {
		const size_t n = (size_t)atol(argv[2]);
		char *buf = malloc(n);
		if (!buf) return 2;
		opt.outfile_name = strcmp(argv[3], "-") ? argv[3] : NULL;
		opt.path = argv[4];
		opt.filename_file = argv[5];
		const size_t len = mc_result_path(&opt, buf, n, ".admix.K=%d.%s", 3, "first.txt");
		printf("%zu\n%s\n", len, buf);
		snprintf(buf + len, n - len, ".second");
		printf("%s\n", buf);
		snprintf(buf + len, n - len, "_third_and_longer_%d.popq", 12);
		printf("%s\n", buf);
		free(buf);
		return 0;
	}
	if (argc == 4 && !strcmp(argv[1], "open")) {
		FILE *fp = mc_open_result(argv[2], argv[3], "w");
		printf("%s\n", fp ? "open" : "NULL");
		if (fp) { fprintf(fp, "written\n"); if (mc_close_result(fp)) return 3; }
		return 0;
	}
	if (argc == 4 && !strcmp(argv[1], "slurp")) {
		char *buf;
		size_t n = 0;
		const int rc = mc_slurp(argv[2], argv[3], &buf, &n);
		printf("%d %zu\n", rc, n);
		if (!rc && (strlen(buf) > n || buf[n])) return 3;	/* NUL-terminated */
		free(buf);
		return 0;
	}
	if (argc == 3 && !strcmp(argv[1], "lines")) {
		char *buf;
		size_t n, lines = 0;
		mc_lines it;
		if (mc_slurp("files_host_driver.c", argv[2], &buf, &n)) return 2;
		for (mc_lines_start(&it, buf, n); mc_lines_next(&it);) lines++;
		printf("%zu\n", lines);
		for (mc_lines_start(&it, buf, n); mc_lines_next(&it);)
			printf("%td %td %td %td\n", it.line - buf, it.first - buf, it.end - buf, it.stop - buf);
		if (mc_lines_next(&it)) return 3;	/* (exhausted stays exhausted) */
		free(buf);
		return 0;
	}
	if (argc >= 4 && !strcmp(argv[1], "copy")) {
		int *map = map_of(argc - 4, argv + 4);
		if (!map) return 2;
		printf("%d\n", mc_copy_kept_lines("files_host_driver.c", argv[2], argv[3], map, argc - 4));
		free(map);
		return 0;
	}
	if (argc >= 4 && !strcmp(argv[1], "lists")) {
		int *map = map_of(argc - 4, argv + 4);
		if (!map) return 2;
		opt.outfile_name = argv[2];
		printf("%d\n", mc_write_kept_lists(&opt, "files_host_driver.c", ".kept", atoi(argv[3]), argc - 4, map, print_entry, "e"));
		free(map);
		return 0;
	}
	fprintf(stderr, "usage: files_host_driver path | open | slurp | lines | copy | lists ... (see the head of tests/files_host_driver.c)\n");
	return 2;
}

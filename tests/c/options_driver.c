/* options_driver.c -- the benchmark driver's option parser as a stand-alone program, for runs under the host sanitizers: it links
 * sbh_options.c, sbh_mg.c (for sbh_mg_levels) and sbh_base.c (for the parameter reader) and no device library (build with
 * -ffunction-sections -Wl,--gc-sections: what those files hold beside is dropped).  Reads command lines from stdin, one per line,
 * the words separated by tabs, and prints for each the status, the action, the parsed fields and the message.
 */
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

int main(void)
{
  char line[MAXLINE];
  int n = 0;
  while (fgets(line, sizeof line, stdin)) {
    char* argv[256] = { "sparseBench" };
    int argc = 1;
    line[strcspn(line, "\n")] = '\0';
    for (char* w = strtok(line, "\t"); w && argc < 255; w = strtok(NULL, "\t")) argv[argc++] = w;
    argv[argc] = NULL;
    Parameter param;
    sbh_options o;
    char msg[MAXLINE];
    initParameter(&param);
    const int status = sbh_parse_options(argc, argv, &param, &o, msg, sizeof msg);
    printf("%d: status %d action %d type %d precond %d %d %d %d byP %d optind %d of %d -m %s grid %d %d %d %s%s", ++n, status, o.action, o.type,
        o.precond.kind, o.precond.levels, o.precond.steps, o.precond.coarse, o.byP, o.optind, argc, param.filename, param.nx, param.ny, param.nz,
        o.toStdout ? "stdout " : "", status ? msg : "\n");
  }
  return EXIT_SUCCESS;
}

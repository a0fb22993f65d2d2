"""Write a stand-alone C++ program (its own main) that makes every rejected call of
tests/test_eval_args.py through the C entries and checks the return code and gpt_last_error, for
running the host files of the stored-sample evaluation entries under the host sanitizers:

    make -C gpt_amd/csrc eval-args-san

writes the program, compiles it and api_pred, api_gpnt, api_cls and api_predictive with
-Xarch_host -fsanitize=address,undefined, links them with the library's other objects and runs it.

The program needs no device: every call returns before its first device call.  It prints the
number of calls made and of those that returned another code or message, and exits with 1 when
there is one; a sanitizer report ends it at the fault."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_eval_args as T  # noqa: E402
from test_julia_shim import header_prototypes  # noqa: E402


def literal(v, ctype, arrays):
    if v is None:
        return "nullptr"
    if isinstance(v, np.ndarray):
        arrays.append("  static int32_t a%d[] = {%s};" % (len(arrays), ", ".join(map(str, v.ravel(order="F")))))
        return "(%s)a%d" % (ctype, len(arrays) - 1)
    if isinstance(v, float):
        if math.isnan(v):
            return "NAN"
        return ("-" if v < 0 else "") + "INFINITY" if math.isinf(v) else repr(v)
    return "(%s)%dLL" % (ctype, v)


def main(out):
    protos = header_prototypes()
    arrays, calls = [], []
    for entry, order in T.ENTRIES.items():
        for over, text in T.BAD[entry]:
            p = dict(T._problem(), **over)
            args = [literal(p[name], ctype, arrays) if name in p else "(%s)dummy" % ctype
                    for name, ctype in zip(order.split(), protos[entry][1])]
            calls.append('  expect(%s(%s), "%s", "%s");' % (entry, ", ".join(args), entry, text))
    src = ['#include <cmath>', '#include <cstdio>', '#include <cstring>', '#include "gptsgld.h"', '',
           'static int bad = 0, made = 0;', 'static double dummy[256];',
           'static void expect(int rc, const char* entry, const char* text) {', '  ++made;',
           '  if (rc == GPT_ERR_BAD_DIMS && std::strstr(gpt_last_error(), text)) return;',
           '  std::printf("%s: rc %d, \\"%s\\" instead of \\"%s\\"\\n", entry, rc, gpt_last_error(), text);',
           '  ++bad;', '}', '', 'int main() {', '  for (double& d : dummy) d = 1.0;'] + arrays + calls + [
           '  std::printf("%d rejected calls, %d wrong\\n", made, bad);', '  return bad != 0;', '}', '']
    with open(out, "w") as f:
        f.write("\n".join(src))
    print("%d calls written to %s" % (len(calls), out))


if __name__ == "__main__":
    main(sys.argv[1])

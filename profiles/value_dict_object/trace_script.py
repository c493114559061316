"""The value dictionaries' three owners in one small run, for a kernel trace: an 82^3 Poisson box with gamg -- the pattern's first
solve, a warm step, a step on other coefficients -- and then a Jacobi solve with the inverse diagonal as codes."""
import os

import numpy as np

import pfemfort_amd as pf
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H

dm, conn, xyz, edof = D._setup(pf.POISSON_TET, H.gen_box_tets(-1, 1, 82, -1, 1, 82, -1, 1, 82))
s = pf.PetscSolver()
s.initialise(dm.size_global, dm.size_global)
s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
s.buildPattern()
s.setPreconditioner("gamg")
s.setTolerances(rtol=1e-6, maxits=5000)
for what, ed in (("first", H.POISSON_ELEMDATA), ("warm", H.POISSON_ELEMDATA), ("other coefficients", np.array([1.3, 0.7, 2.1]))):
    s.assemble(ed, H.TIMEDATA)
    its, reason, _ = s.factoriseAndSolve()
    print(what, "its", its, "reason", reason, "value dictionaries", s.amgValueDictionaries(), "column codes", s.amgCycle()["column_codes"], flush=True)
os.environ["PFEM_DINV_CODES_MIN_ROWS"] = "1"
s.setPreconditioner("jacobi")
s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
its, reason, _ = s.factoriseAndSolve()
print("jacobi its", its, "reason", reason, "matrix dictionary", s.spmvValueDictionary(), flush=True)
s.free()

# At 82^3 the row form is in effect, whose values are never codes: the same run once more with the 4-row groups asked for, so that
# the matrix's own dictionary (build, codes written by the assembly, a miss and the rebuild) and the diagonal's are in the listing.
del os.environ["PFEM_DINV_CODES_MIN_ROWS"]
s = pf.PetscSolver()
s.initialise(dm.size_global, dm.size_global)
s.uploadMesh(pf.POISSON_TET, conn, xyz, edof, dm.solnApplied)
s.setSpmvFormat("grouped")
s.buildPattern()
s.setPreconditioner("gamg")
s.setTolerances(rtol=1e-6, maxits=5000)
for what, ed in (("grouped first", H.POISSON_ELEMDATA), ("grouped warm", H.POISSON_ELEMDATA), ("grouped warm 2", H.POISSON_ELEMDATA),
                 ("grouped other coefficients", np.array([1.3, 0.7, 2.1])), ("grouped other coefficients, warm", np.array([1.3, 0.7, 2.1]))):
    s.assemble(ed, H.TIMEDATA)
    its, reason, _ = s.factoriseAndSolve()
    print(what, "its", its, "reason", reason, "rows to the lane", s.spmvRowGroup(), "matrix dictionary", s.spmvValueDictionary(), "value dictionaries",
          s.amgValueDictionaries(), flush=True)
os.environ["PFEM_DINV_CODES_MIN_ROWS"] = "1"
s.setPreconditioner("jacobi")
s.assemble(H.POISSON_ELEMDATA, H.TIMEDATA)
its, reason, _ = s.factoriseAndSolve()
print("grouped jacobi its", its, "reason", reason, "matrix dictionary", s.spmvValueDictionary(), flush=True)
s.free()
